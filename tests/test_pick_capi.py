"""CPU tests of vr_pick at the C ABI (no device): the symbol is exported and bound, the record
is 64 bytes in every mirror, and the argument checks that come before any device work fail
with VR_E_INVALID and a message that names vr_pick."""
from __future__ import annotations

import ctypes
import os

import numpy as np

import voxelraymarcher_amd as vr
from tests import pick_ref
from voxelraymarcher_amd import _capi


def _last_error() -> str:
    return vr.lib().vr_last_error().decode()


def test_symbol_and_record():
    lib = vr.lib()
    assert "vr_pick" in _capi.SIGNATURES and lib.vr_pick.argtypes == _capi.SIGNATURES["vr_pick"][1]
    assert ctypes.sizeof(_capi.VrHit) == 64 and vr.HIT_DTYPE.itemsize == 64
    assert vr.HIT_DTYPE == pick_ref.HIT_DTYPE
    for name, typ in _capi.VrHit._fields_:
        assert vr.HIT_DTYPE.fields[name][1] == getattr(_capi.VrHit, name).offset
        assert vr.HIT_DTYPE.fields[name][0].itemsize == ctypes.sizeof(typ)
    header = open(os.path.join(os.path.dirname(_capi.HERE), "include", "vr.h")).read()
    for name, value in (("MISS", 0), ("VOXEL", 1), ("NEVER", 2), ("OUTSIDE", 3)):
        assert f"#define VR_HIT_{name}" in header
        line = [ln for ln in header.splitlines() if ln.startswith(f"#define VR_HIT_{name}")][0]
        assert line.split()[2] == f"{value}u"
        assert int(vr.HitStatus[name]) == value == getattr(pick_ref, name)
    assert callable(vr.pick) and hasattr(vr.DeviceScene, "pick")
    mirror = open(os.path.join(os.path.dirname(_capi.HERE), "include", "vr.hpp")).read()
    assert "vr_pick(" in mirror


def _call(lib, s, cam, tr, W, H, px, py, n, hits, algo=1):
    return lib.vr_pick(s, algo, cam, tr, 1, W, H, px, py, n, 0, hits, 0, None)


def test_invalid_arguments_name_vr_pick():
    lib = vr.lib()
    cam = ctypes.pointer(_capi.VrCamera())
    tr = _capi.f3((0.0, 0.0, 0.0))
    q = np.zeros(4, dtype=np.uint32)
    hits = np.zeros(4, dtype=vr.HIT_DTYPE)
    p, h = q.ctypes.data_as(ctypes.c_void_p), hits.ctypes.data_as(ctypes.c_void_p)
    # (every check below comes before the scene is looked at: any non-null handle will do)
    fake = ctypes.create_string_buffer(256)

    def invalid(rc, word):
        assert rc == -1 and "vr_pick" in _last_error() and word in _last_error(), _last_error()

    invalid(_call(lib, None, cam, tr, 8, 8, p, p, 1, h), "NULL")
    invalid(_call(lib, fake, None, tr, 8, 8, p, p, 1, h), "NULL")
    invalid(_call(lib, fake, cam, None, 8, 8, p, p, 1, h), "NULL")
    for a, b, c in ((None, p, h), (p, None, h), (p, p, None)):
        invalid(_call(lib, fake, cam, tr, 8, 8, a, b, 1, c), "NULL")
    for W, H in ((0, 8), (8, 0), (65537, 8), (8, 65537)):
        invalid(_call(lib, fake, cam, tr, W, H, p, p, 1, h), "size")
    invalid(_call(lib, fake, cam, tr, 8, 8, p, p, 1 << 31, h), "many")
    invalid(_call(lib, fake, cam, tr, 8, 8, p, p, 1, h, algo=7), "algorithm")
    # device hits must be 16-byte aligned: checked on the pointer alone, beside the other checks
    off8 = ctypes.c_void_p(hits.ctypes.data + 8)
    invalid(lib.vr_pick(fake, 1, cam, tr, 1, 8, 8, p, p, 1, 0, off8, 1, None), "aligned")
    assert not hits.tobytes().strip(b"\0")                                   # nothing was written
    assert _call(lib, fake, cam, tr, 8, 8, None, None, 0, None) == 0          # n == 0: nothing to do
    assert _call(lib, fake, cam, tr, 65536, 65536, p, p, 0, h) == 0
