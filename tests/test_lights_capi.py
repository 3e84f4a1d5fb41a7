"""CPU tests of vr_shade_lights at the C ABI (no device), in the manner of tests/test_shade_capi.py:
the symbol is exported and bound with the header's signature, the Python and C++ mirrors exist,
and the argument checks that come before any device work fail with VR_E_INVALID, a message that
names the function, and both output buffers untouched."""
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


def test_symbol_and_signature():
    lib = vr.lib()
    assert "vr_shade_lights" in _capi.SIGNATURES
    res, args = _capi.SIGNATURES["vr_shade_lights"]
    assert lib.vr_shade_lights.argtypes == args and lib.vr_shade_lights.restype == res == c_int
    # scene, algo, lights, n_lights, ambient, translation, scale, rays, n, inputs_on_device, colors,
    # hits, outputs_on_device, order, stream
    assert args == [c_void_p, c_int, POINTER(_capi.VrLighting), c_size_t, POINTER(c_float), POINTER(c_float), c_uint32,
                    c_void_p, c_size_t, c_int, c_void_p, c_void_p, c_int, c_uint32, c_void_p]
    header = _read("include", "vr.h")
    m = re.search(r"^int vr_shade_lights\(([^;]*)\);", header, flags=re.M | re.S)
    assert m is not None
    params = [re.sub(r"/\*.*?\*/", "", p).strip() for p in re.sub(r"\s+", " ", m.group(1)).split(",")]
    assert params == ["const vr_scene* s", "vr_algo algo", "const vr_lighting* lights", "size_t n_lights",
                      "const float ambient[3]", "const float translation[3]", "uint32_t scale", "const vr_ray* rays",
                      "size_t n", "int inputs_on_device", "uint32_t* colors", "vr_hit* hits", "int outputs_on_device",
                      "uint32_t order", "void* stream"]
    assert re.search(r"^#define VR_MAX_LIGHTS 64u$", header, flags=re.M) and _capi.VR_MAX_LIGHTS == 64
    assert header.index("int vr_shade(") < header.index("int vr_shade_lights(") < header.index("int vr_camera_rays(")
    assert callable(vr.shade_lights) and callable(vr.render_lights) and hasattr(vr.DeviceScene, "shade_lights")
    mirror = _read("include", "vr.hpp")
    assert "vr_shade_lights(" in mirror and re.search(r"std::vector<uint32_t> shadeLights\(", mirror)


def test_shade_lights_invalid_arguments_name_vr_shade_lights():
    lib = vr.lib()
    tr = _capi.f3((0.0, 0.0, 0.0))
    amb = _capi.f3((0.25, 0.25, 0.25))
    lights = (_capi.VrLighting * 65)(*[vr.setup_constant_values() for _ in range(65)])
    rays = np.zeros(4, dtype=vr.RAY_DTYPE)
    hits = np.zeros(4, dtype=vr.HIT_DTYPE)
    colors = np.zeros(5, dtype=np.uint32)
    r, h, c = (a.ctypes.data_as(c_void_p) for a in (rays, hits, colors))
    # (every check below comes before the scene is looked at: any non-null handle will do)
    fake = ctypes.create_string_buffer(256)

    def call(s=fake, algo=1, li=lights, nl=2, am=amb, t=tr, rr=r, n=1, cc=c, hh=h, order=0, in_dev=0, out_dev=0):
        return lib.vr_shade_lights(s, algo, li, nl, am, t, 1, rr, n, in_dev, cc, hh, out_dev, order, None)

    def invalid(rc, word):
        assert rc == -1 and "vr_shade_lights" in _last_error() and word in _last_error(), _last_error()

    invalid(call(s=None), "NULL")
    invalid(call(t=None), "NULL")
    invalid(call(li=None), "NULL")
    invalid(call(li=None, nl=1, am=None), "NULL")
    invalid(call(nl=65), "VR_MAX_LIGHTS")
    invalid(call(nl=65, n=0), "VR_MAX_LIGHTS")
    invalid(call(nl=1 << 40), "VR_MAX_LIGHTS")
    invalid(call(rr=None), "NULL")
    invalid(call(cc=None), "NULL")
    invalid(call(cc=None, hh=None), "NULL")
    invalid(call(n=1 << 31), "many")
    invalid(call(n=1 << 40), "many")
    invalid(call(algo=7), "algorithm")
    for order in (3, 7, 0xFFFFFFFF):
        invalid(call(order=order), "order")
    # device arrays: rays and hits 16-byte aligned, colors 4-byte aligned (checked on the pointer alone)
    invalid(call(rr=c_void_p(rays.ctypes.data + 4), in_dev=1), "aligned")
    invalid(call(hh=c_void_p(hits.ctypes.data + 8), out_dev=1), "aligned")
    for off in (1, 2, 3):
        invalid(call(cc=c_void_p(colors.ctypes.data + off), out_dev=1), "aligned")
        invalid(call(cc=c_void_p(colors.ctypes.data + off), hh=None, out_dev=1), "aligned")
    assert not hits.tobytes().strip(b"\0") and not colors.any()     # nothing was written
    # n == 0: nothing to do -- with and without lights, ambient and records, under every order
    assert call(rr=None, cc=None, hh=None, n=0) == 0
    assert call(li=None, nl=0, am=None, rr=None, cc=None, hh=None, n=0) == 0
    assert call(nl=64, n=0) == 0
    for order in (0, 1, 2):
        assert call(n=0, order=order) == 0
        assert call(n=0, hh=None, am=None, order=order) == 0
