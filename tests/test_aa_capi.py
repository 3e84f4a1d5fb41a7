"""CPU tests of vr_aa_fine_words, vr_resolve and vr_render_aa at the C ABI (no device), in the manner
of tests/test_lights_capi.py: the symbols are exported and bound with the header's signatures, the
Python and C++ mirrors exist, and every argument check that comes before any device work fails
with VR_E_INVALID and a message that names the function."""
from __future__ import annotations

import ctypes
import os
import re
from ctypes import POINTER, c_float, c_int, c_uint32, c_uint64, c_void_p

import numpy as np
import pytest

import voxelraymarcher_amd as vr
from voxelraymarcher_amd import _capi


def _last_error() -> str:
    return vr.lib().vr_last_error().decode()


def _read(*parts) -> str:
    return open(os.path.join(os.path.dirname(_capi.HERE), *parts)).read()


def _params(header: str, decl: str):
    m = re.search(r"^" + re.escape(decl) + r"\(([^;]*)\);", header, flags=re.M | re.S)
    assert m is not None, decl
    return [re.sub(r"/\*.*?\*/", "", p).strip() for p in re.sub(r"\s+", " ", m.group(1)).split(",")]


def test_symbols_and_signatures():
    lib = vr.lib()
    for name in ("vr_aa_fine_words", "vr_resolve", "vr_render_aa"):
        res, args = _capi.SIGNATURES[name]
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res
    assert _capi.SIGNATURES["vr_aa_fine_words"] == (c_uint64, [c_uint32, c_uint32, c_uint32])
    assert _capi.SIGNATURES["vr_resolve"] == (c_int, [c_void_p, c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p])
    assert _capi.SIGNATURES["vr_render_aa"] == (
        c_int, [c_void_p, c_int, POINTER(_capi.VrCamera), POINTER(_capi.VrLighting), POINTER(c_float), c_uint32, c_uint32,
                c_uint32, c_uint32, c_uint32, c_uint32, c_void_p, c_uint64, c_void_p, c_void_p, c_void_p])
    header = _read("include", "vr.h")
    assert _params(header, "uint64_t vr_aa_fine_words") == ["uint32_t width", "uint32_t rows", "uint32_t samples"]
    assert _params(header, "int vr_resolve") == ["const uint32_t* fine_dev", "uint32_t width", "uint32_t rows",
                                                 "uint32_t samples", "uint32_t* out_dev", "uint8_t* out_rgb8_dev",
                                                 "void* stream"]
    assert _params(header, "int vr_render_aa") == [
        "const vr_scene* s", "vr_algo algo", "const vr_camera* cam", "const vr_lighting* lit", "const float translation[3]",
        "uint32_t scale", "uint32_t width", "uint32_t height", "uint32_t samples", "uint32_t row_begin", "uint32_t row_end",
        "uint32_t* fine_dev", "uint64_t fine_words", "uint32_t* out_dev", "uint8_t* out_rgb8_dev", "void* stream"]
    assert callable(vr.resolve) and callable(vr.render_aa) and callable(vr.aa_fine_words)
    mirror = _read("include", "vr.hpp")
    assert "vr_render_aa(" in mirror and "vr_resolve(" in mirror and "vr_aa_fine_words(" in mirror


def test_aa_fine_words():
    f = vr.lib().vr_aa_fine_words
    assert f(32, 24, 1) == 32 * 24 and f(32, 24, 2) == 64 * 48 and f(32, 24, 4) == 128 * 96 and f(32, 24, 8) == 256 * 192
    assert f(1920, 1080, 4) == 7680 * 4320
    assert f(1, 1, 8) == 64 and f(65536, 65536, 1) == 1 << 32 and f(8192, 8192, 8) == 1 << 32
    assert f(32768, 1, 2) == 65536 * 2 and f(1, 32768, 2) == 2 * 65536
    assert f(32, 0, 4) == 0                                   # an empty row range: no words
    # 0 for what vr_render_aa rejects
    for S in (0, 3, 5, 6, 7, 9, 16, 0xFFFFFFFF):
        assert f(32, 24, S) == 0, S
    assert f(0, 24, 2) == 0 and f(65537, 1, 1) == 0 and f(1, 65537, 1) == 0
    assert f(32769, 1, 2) == 0 and f(1, 32769, 2) == 0 and f(16385, 1, 4) == 0 and f(1, 8193, 8) == 0
    assert f(0xFFFFFFFF, 0xFFFFFFFF, 8) == 0
    assert vr.aa_fine_words(32, 24, 2) == 3072 and vr.aa_fine_words(32, 24, 3) == 0 and vr.aa_fine_words(-1, 2, 2) == 0


def invalid(rc, who, word):
    assert rc == -1 and who in _last_error() and word in _last_error(), (rc, _last_error())


def test_resolve_invalid_arguments_name_vr_resolve():
    lib = vr.lib()
    fine = np.zeros(64 * 64 + 4, dtype=np.uint32)
    out = np.full(64, 0xABABABAB, dtype=np.uint32)
    rgb = np.full(64 * 3, 0xAB, dtype=np.uint8)
    f, o, r = (a.ctypes.data_as(c_void_p) for a in (fine, out, rgb))

    def call(ff=f, w=8, rows=8, S=2, oo=o, rr=r):
        return lib.vr_resolve(ff, w, rows, S, oo, rr, None)

    invalid(call(ff=None), "vr_resolve", "NULL")
    invalid(call(oo=None, rr=None), "vr_resolve", "NULL")
    for S in (0, 3, 5, 16, 0xFFFFFFFF):
        invalid(call(S=S), "vr_resolve", "samples")
    for w, rows in ((0, 8), (8, 0), (65537, 8), (8, 65537), (0xFFFFFFFF, 1)):
        invalid(call(w=w, rows=rows), "vr_resolve", "size")
    for w, rows, S in ((32769, 1, 2), (1, 32769, 2), (16385, 1, 4), (1, 8193, 8), (65536, 65536, 2)):
        invalid(call(w=w, rows=rows, S=S), "vr_resolve", "large")
    for off in (1, 2, 3):
        invalid(call(ff=c_void_p(fine.ctypes.data + off)), "vr_resolve", "aligned")
        invalid(call(oo=c_void_p(out.ctypes.data + off)), "vr_resolve", "aligned")
    assert (out == 0xABABABAB).all() and (rgb == 0xAB).all()     # nothing was written


def test_render_aa_invalid_arguments_name_vr_render_aa():
    lib = vr.lib()
    tr = _capi.f3((0.0, 0.0, 0.0))
    cam = vr.Camera.reference(32, 24)
    lit = vr.setup_constant_values()
    fine = np.zeros(64 * 48 + 4, dtype=np.uint32)
    out = np.full(32 * 24, 0xABABABAB, dtype=np.uint32)
    rgb = np.full(32 * 24 * 3, 0xAB, dtype=np.uint8)
    f, o, r = (a.ctypes.data_as(c_void_p) for a in (fine, out, rgb))
    # (every check below comes before the scene is looked at: any non-null handle will do)
    fake = ctypes.create_string_buffer(256)
    C, L = ctypes.byref(cam.raw), ctypes.byref(lit)

    def call(s=fake, algo=1, c=C, li=L, t=tr, w=32, h=24, S=2, r0=0, r1=24, ff=f, words=64 * 48, oo=o, rr=r):
        return lib.vr_render_aa(s, algo, c, li, t, 12, w, h, S, r0, r1, ff, words, oo, rr, None)

    who = "vr_render_aa"
    for null in ("s", "c", "li", "t", "ff"):
        invalid(call(**{null: None}), who, "NULL")
    invalid(call(oo=None, rr=None), who, "NULL")
    for S in (0, 3, 5, 6, 7, 16, 0xFFFFFFFF):
        invalid(call(S=S), who, "samples")
    for w, h in ((0, 24), (32, 0), (65537, 24), (32, 65537)):
        invalid(call(w=w, h=h, r1=0), who, "size")
    for w, h, S in ((32769, 24, 2), (32, 32769, 2), (16385, 24, 4), (32, 8193, 8)):
        invalid(call(w=w, h=h, S=S, r1=0), who, "large")
    for r0, r1 in ((5, 4), (0, 25), (25, 25), (24, 23), (0, 0xFFFFFFFF)):
        invalid(call(r0=r0, r1=r1), who, "row range")
    invalid(call(words=64 * 48 - 1), who, "fine_words")
    invalid(call(words=0), who, "fine_words")
    invalid(call(S=4), who, "fine_words")                   # the same buffer is too small at S = 4
    invalid(call(r0=0, r1=12, words=64 * 24 - 1), who, "fine_words")
    invalid(call(algo=7), who, "algorithm")
    invalid(call(algo=-1), who, "algorithm")
    for off in (1, 2, 3):
        invalid(call(ff=c_void_p(fine.ctypes.data + off)), who, "aligned")
        invalid(call(oo=c_void_p(out.ctypes.data + off)), who, "aligned")
    # an empty row range is VR_OK and does nothing, with any buffer size
    assert call(r0=0, r1=0, words=0) == 0 and call(r0=24, r1=24, words=0) == 0 and call(r0=7, r1=7) == 0
    assert call(r0=7, r1=7, oo=None) == 0 and call(r0=7, r1=7, rr=None) == 0
    assert (out == 0xABABABAB).all() and (rgb == 0xAB).all() and not fine.any()      # nothing was written


def test_python_wrappers_refuse_before_the_library():
    with pytest.raises(ValueError):
        vr.render_lights(None, vr.RayMarchAlgorithm.ORIGINAL, None, None, [], 32, 24, samples=3)
