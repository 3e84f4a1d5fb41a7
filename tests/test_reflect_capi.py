"""CPU tests of vr_bounce_rays and vr_shade_lights_reflect at the C ABI (no device), in the manner of
tests/test_ao_capi.py: the symbols are exported and bound with the header's signatures, stand in the
header where they belong, the Python and C++ mirrors exist, and the argument checks that come before
any device work fail with VR_E_INVALID, a message that names the function, and the output buffers
untouched."""
from __future__ import annotations

import ctypes
import inspect
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
    res, args = _capi.SIGNATURES["vr_bounce_rays"]
    assert lib.vr_bounce_rays.argtypes == args and lib.vr_bounce_rays.restype == res == c_int
    assert args == [c_int, POINTER(c_float), c_uint32, c_void_p, c_void_p, c_size_t, c_int, c_void_p, c_int, c_void_p]
    assert _params(header, "vr_bounce_rays") == ["int device", "const float translation[3]", "uint32_t scale", "const vr_ray* rays",
                                                 "const vr_hit* hits", "size_t n", "int inputs_on_device", "vr_ray* out",
                                                 "int outputs_on_device", "void* stream"]
    res, args = _capi.SIGNATURES["vr_shade_lights_reflect"]
    assert lib.vr_shade_lights_reflect.argtypes == args and lib.vr_shade_lights_reflect.restype == res == c_int
    # every argument of vr_shade_lights_ao, in its order, then the four of the reflection
    assert args == _capi.SIGNATURES["vr_shade_lights_ao"][1] + [c_uint32] * 4
    assert _params(header, "vr_shade_lights_reflect") == _params(header, "vr_shade_lights_ao") + [
        "uint32_t reflectivity", "uint32_t bounces", "uint32_t mirror_mask", "uint32_t mirror_value"]
    assert re.search(r"^#define VR_MAX_BOUNCES 4u$", header, flags=re.M) and _capi.VR_MAX_BOUNCES == vr.MAX_BOUNCES == 4
    order = [header.index(s) for s in ("int vr_shade_lights_ao(", "int vr_bounce_rays(", "int vr_shade_lights_reflect(",
                                       "int vr_camera_rays(")]
    assert order == sorted(order)
    # the header says what an all-NaN ray does, and what the call allocates
    block = header[header.index("int vr_shade_lights_ao("):header.index("int vr_camera_rays(")]
    assert "NOT harmless" in block and "VR_HIT_NEVER" in block and "allocates" in block
    assert callable(vr.bounce_rays)
    for fn in (vr.shade_lights, vr.DeviceScene.shade_lights, vr.render_lights):
        p = inspect.signature(fn).parameters
        assert {"reflect", "bounces", "mirror"} <= set(p) and p["bounces"].default == 1 and p["mirror"].default is None, fn
    assert list(inspect.signature(vr.bounce_rays).parameters) == ["rays", "hits", "info", "device", "stream"]
    mirror = _read("include", "vr.hpp")
    assert "vr_bounce_rays(" in mirror and re.search(r"std::vector<vr_ray> bounceRays\(", mirror)
    assert "vr_shade_lights_reflect(" in mirror and re.search(r"std::vector<uint32_t> shadeLightsReflect\(", mirror)


def test_bounce_rays_invalid_arguments_name_vr_bounce_rays():
    lib = vr.lib()
    tr = _capi.f3((0.0, 0.0, 0.0))
    rays = np.zeros(4, dtype=vr.RAY_DTYPE)
    hits = np.zeros(4, dtype=vr.HIT_DTYPE)
    out = np.full(5 * 8, 0xABABABAB, dtype=np.uint32)
    r, h, o = (x.ctypes.data_as(c_void_p) for x in (rays, hits, out))

    def call(device=0, t=tr, rr=r, hh=h, n=1, oo=o, in_dev=0, out_dev=0):
        return lib.vr_bounce_rays(device, t, 1, rr, hh, n, in_dev, oo, out_dev, None)

    def invalid(rc, word):
        assert rc == -1 and "vr_bounce_rays" in _last_error() and word in _last_error(), _last_error()

    invalid(call(t=None), "NULL")
    invalid(call(t=None, n=0), "NULL")
    invalid(call(rr=None), "NULL")
    invalid(call(hh=None), "NULL")
    invalid(call(oo=None), "NULL")
    invalid(call(n=1 << 31), "many")
    invalid(call(n=1 << 40), "many")
    invalid(call(device=-1), "device")
    invalid(call(device=64), "device")
    invalid(call(device=64, n=0), "device")
    for off in (4, 8, 12, 1):
        invalid(call(rr=c_void_p(rays.ctypes.data + off), in_dev=1), "aligned")
        invalid(call(hh=c_void_p(hits.ctypes.data + off), in_dev=1), "aligned")
        invalid(call(oo=c_void_p(out.ctypes.data + off), out_dev=1), "aligned")
    assert (out == 0xABABABAB).all()                # nothing was written
    assert call(rr=None, hh=None, oo=None, n=0) == 0 and call(n=0) == 0


def test_shade_lights_reflect_invalid_arguments_name_vr_shade_lights_reflect():
    lib = vr.lib()
    tr = _capi.f3((0.0, 0.0, 0.0))
    amb = _capi.f3((0.25, 0.25, 0.25))
    lights = (_capi.VrLighting * 65)(*[vr.setup_constant_values() for _ in range(65)])
    rays = np.zeros(4, dtype=vr.RAY_DTYPE)
    hits = np.zeros(4, dtype=vr.HIT_DTYPE)
    colors = np.zeros(5, dtype=np.uint32)
    ao = np.zeros(5, dtype=np.uint32)
    r, h, c, a = (x.ctypes.data_as(c_void_p) for x in (rays, hits, colors, ao))
    fake = ctypes.create_string_buffer(256)      # (every check below comes before the scene is looked at)

    def call(s=fake, algo=1, li=lights, nl=2, am=amb, t=tr, rr=r, n=1, cc=c, hh=h, order=0, in_dev=0, out_dev=0, strength=96,
             apply=0, aa=a, k=128, bounces=2, mask=0, value=0):
        return lib.vr_shade_lights_reflect(s, algo, li, nl, am, t, 1, rr, n, in_dev, cc, hh, out_dev, order, None, strength, apply,
                                           aa, k, bounces, mask, value)

    def invalid(rc, word):
        assert rc == -1 and "vr_shade_lights_reflect" in _last_error() and word in _last_error(), _last_error()

    # the three cases of its own, with and without rays
    for k in (256, 1000, 0xFFFFFFFF):
        invalid(call(k=k), "reflectivity")
        invalid(call(k=k, n=0), "reflectivity")
    for b in (5, 64, 0xFFFFFFFF):
        invalid(call(bounces=b), "VR_MAX_BOUNCES")
        invalid(call(bounces=b, n=0, k=0), "VR_MAX_BOUNCES")
    for mask, value in ((0, 1), (1, 2), (0xFFFFFF, 0x1000000), (0xFF00, 0xFF01), (0x7FFFFFFF, 0x80000000)):
        invalid(call(mask=mask, value=value), "mirror_value")
        invalid(call(mask=mask, value=value, n=0), "mirror_value")
    # vr_shade_lights_ao's cases, under this function's name
    invalid(call(strength=256), "ao_strength")
    invalid(call(apply=2), "ao_apply")
    for off in (1, 2, 3):
        invalid(call(aa=c_void_p(ao.ctypes.data + off), out_dev=1), "aligned")
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
    # its siblings still answer under their own names
    assert lib.vr_shade_lights_ao(None, 1, lights, 2, amb, tr, 1, r, 1, 0, c, h, 0, 0, None, 0, 0, None) == -1
    assert "vr_shade_lights_ao:" in _last_error()
    # n == 0: nothing to do, at every depth and with every mirror test that can match
    for bounces in range(5):
        assert call(rr=None, cc=None, hh=None, aa=None, n=0, bounces=bounces) == 0
        assert call(n=0, bounces=bounces, k=255, mask=0xFFFFFF, value=0x123456) == 0 and call(n=0, bounces=bounces, k=0) == 0
