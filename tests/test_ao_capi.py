"""CPU tests of vr_occlusion and vr_shade_lights_ao at the C ABI (no device), in the manner of
tests/test_lights_capi.py: the symbols are exported and bound with the header's signatures, stand
in the header where they belong, the Python and C++ mirrors exist, and the argument checks that
come before any device work fail with VR_E_INVALID, a message that names the function, and the
output buffers untouched."""
from __future__ import annotations

import ctypes
import os
import re
from ctypes import POINTER, c_float, c_int, c_size_t, c_uint32, c_void_p

import numpy as np

import voxelraymarcher_amd as vr
from voxelraymarcher_amd import _capi


def _last_error() -> str:
    return vr.lib().vr_last_error().decode()


def _read(*parts) -> str:
    return open(os.path.join(os.path.dirname(_capi.HERE), *parts)).read()


def _params(header, name):
    m = re.search(r"^int %s\(([^;]*)\);" % name, header, flags=re.M | re.S)
    assert m is not None, name
    return [re.sub(r"/\*.*?\*/", "", p).strip() for p in re.sub(r"\s+", " ", m.group(1)).split(",")]


def test_symbols_and_signatures():
    lib = vr.lib()
    header = _read("include", "vr.h")
    res, args = _capi.SIGNATURES["vr_occlusion"]
    assert lib.vr_occlusion.argtypes == args and lib.vr_occlusion.restype == res == c_int
    assert args == [c_void_p, c_void_p, c_size_t, c_int, c_void_p, c_int, c_void_p]
    assert _params(header, "vr_occlusion") == ["const vr_scene* s", "const vr_hit* hits", "size_t n", "int inputs_on_device",
                                               "uint32_t* ao", "int outputs_on_device", "void* stream"]
    res, args = _capi.SIGNATURES["vr_shade_lights_ao"]
    assert lib.vr_shade_lights_ao.argtypes == args and lib.vr_shade_lights_ao.restype == res == c_int
    # every argument of vr_shade_lights, in its order, then the three of the occlusion
    assert args == _capi.SIGNATURES["vr_shade_lights"][1] + [c_uint32, c_uint32, c_void_p]
    assert args[:7] == [c_void_p, c_int, POINTER(_capi.VrLighting), c_size_t, POINTER(c_float), POINTER(c_float), c_uint32]
    assert _params(header, "vr_shade_lights_ao") == _params(header, "vr_shade_lights") + [
        "uint32_t ao_strength", "uint32_t ao_apply", "uint32_t* ao_out"]
    assert re.search(r"^#define VR_AO_OPEN 255u$", header, flags=re.M) and _capi.VR_AO_OPEN == vr.AO_OPEN == 255
    assert re.search(r"VR_AO_AMBIENT = 0,.*?VR_AO_ALL = 1.*?\} vr_ao_apply;", header, flags=re.S)
    assert (vr.AoApply.AMBIENT, vr.AoApply.ALL) == (_capi.VR_AO_AMBIENT, _capi.VR_AO_ALL) == (0, 1)
    order = [header.index(s) for s in ("int vr_shade_lights(", "int vr_occlusion(", "} vr_ao_apply;", "int vr_shade_lights_ao(",
                                       "int vr_camera_rays(")]
    assert order == sorted(order)
    assert callable(vr.occlusion) and hasattr(vr.DeviceScene, "occlusion")
    import inspect
    for fn in (vr.shade_lights, vr.DeviceScene.shade_lights, vr.render_lights):
        assert {"ao", "ao_apply", "return_ao"} <= set(inspect.signature(fn).parameters), fn
    mirror = _read("include", "vr.hpp")
    assert "vr_occlusion(" in mirror and re.search(r"std::vector<uint32_t> occlusion\(", mirror)
    assert "vr_shade_lights_ao(" in mirror and re.search(r"std::vector<uint32_t> shadeLightsAo\(", mirror)


def test_occlusion_invalid_arguments_name_vr_occlusion():
    lib = vr.lib()
    hits = np.zeros(4, dtype=vr.HIT_DTYPE)
    ao = np.full(5, 0xABABABAB, dtype=np.uint32)
    h, a = hits.ctypes.data_as(c_void_p), ao.ctypes.data_as(c_void_p)
    fake = ctypes.create_string_buffer(256)      # (every check below comes before the scene is looked at)

    def call(s=fake, hh=h, n=1, aa=a, in_dev=0, out_dev=0):
        return lib.vr_occlusion(s, hh, n, in_dev, aa, out_dev, None)

    def invalid(rc, word):
        assert rc == -1 and "vr_occlusion" in _last_error() and word in _last_error(), _last_error()

    invalid(call(s=None), "NULL")
    invalid(call(s=None, n=0), "NULL")
    invalid(call(hh=None), "NULL")
    invalid(call(aa=None), "NULL")
    invalid(call(n=1 << 31), "many")
    invalid(call(n=1 << 40), "many")
    for off in (4, 8, 12, 1):
        invalid(call(hh=c_void_p(hits.ctypes.data + off), in_dev=1), "aligned")
    for off in (1, 2, 3):
        invalid(call(aa=c_void_p(ao.ctypes.data + off), out_dev=1), "aligned")
    assert (ao == 0xABABABAB).all()                 # nothing was written
    assert call(hh=None, aa=None, n=0) == 0 and call(n=0) == 0


def test_shade_lights_ao_invalid_arguments_name_vr_shade_lights_ao():
    lib = vr.lib()
    tr = _capi.f3((0.0, 0.0, 0.0))
    amb = _capi.f3((0.25, 0.25, 0.25))
    lights = (_capi.VrLighting * 65)(*[vr.setup_constant_values() for _ in range(65)])
    rays = np.zeros(4, dtype=vr.RAY_DTYPE)
    hits = np.zeros(4, dtype=vr.HIT_DTYPE)
    colors = np.zeros(5, dtype=np.uint32)
    ao = np.zeros(5, dtype=np.uint32)
    r, h, c, a = (x.ctypes.data_as(c_void_p) for x in (rays, hits, colors, ao))
    fake = ctypes.create_string_buffer(256)

    def call(s=fake, algo=1, li=lights, nl=2, am=amb, t=tr, rr=r, n=1, cc=c, hh=h, order=0, in_dev=0, out_dev=0, strength=96,
             apply=0, aa=a):
        return lib.vr_shade_lights_ao(s, algo, li, nl, am, t, 1, rr, n, in_dev, cc, hh, out_dev, order, None, strength, apply, aa)

    def invalid(rc, word):
        assert rc == -1 and "vr_shade_lights_ao" in _last_error() and word in _last_error(), _last_error()

    # the two cases of its own, with and without rays
    for strength in (256, 1000, 0xFFFFFFFF):
        invalid(call(strength=strength), "ao_strength")
        invalid(call(strength=strength, n=0), "ao_strength")
    for apply in (2, 7, 0xFFFFFFFF):
        invalid(call(apply=apply), "ao_apply")
        invalid(call(apply=apply, aa=None, strength=0), "ao_apply")
    for off in (1, 2, 3):
        invalid(call(aa=c_void_p(ao.ctypes.data + off), out_dev=1), "aligned")
    # vr_shade_lights' cases, under this function's name
    invalid(call(s=None), "NULL")
    invalid(call(t=None), "NULL")
    invalid(call(li=None), "NULL")
    invalid(call(nl=65), "VR_MAX_LIGHTS")
    invalid(call(rr=None), "NULL")
    invalid(call(cc=None), "NULL")
    invalid(call(n=1 << 31), "many")
    invalid(call(algo=7), "algorithm")
    invalid(call(order=3), "order")
    invalid(call(rr=c_void_p(rays.ctypes.data + 4), in_dev=1), "aligned")
    invalid(call(hh=c_void_p(hits.ctypes.data + 8), out_dev=1), "aligned")
    invalid(call(cc=c_void_p(colors.ctypes.data + 2), out_dev=1), "aligned")
    assert not hits.tobytes().strip(b"\0") and not colors.any() and not ao.any()     # nothing was written
    # vr_shade_lights still answers under its own name
    assert lib.vr_shade_lights(None, 1, lights, 2, amb, tr, 1, r, 1, 0, c, h, 0, 0, None) == -1
    assert "vr_shade_lights:" in _last_error()
    # n == 0: nothing to do, in both modes, with and without ao_out
    for apply in (0, 1):
        assert call(rr=None, cc=None, hh=None, aa=None, n=0, apply=apply) == 0
        assert call(n=0, apply=apply, strength=255) == 0 and call(n=0, apply=apply, strength=0) == 0
