"""CPU tests of vr_atmosphere_default, vr_atmosphere_apply and vr_shade_lights_atmosphere at the C ABI
(no device), in the manner of tests/test_reflect_capi.py: the symbols are exported and bound with the
header's signatures, stand in the header where they belong, the Python and C++ mirrors exist, and the
argument checks that come before any device work fail with VR_E_INVALID, a message that names the
function, and the output buffers untouched."""
from __future__ import annotations

import ctypes
import inspect
import os
import re
from ctypes import POINTER, c_float, c_int, c_size_t, c_uint32, c_void_p

import numpy as np
import pytest

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
    for name in ("vr_atmosphere_default", "vr_atmosphere_apply", "vr_shade_lights_atmosphere"):
        res, args = _capi.SIGNATURES[name]
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res == c_int
    A = POINTER(_capi.VrAtmosphere)
    assert _capi.SIGNATURES["vr_atmosphere_default"][1] == [A]
    assert _capi.SIGNATURES["vr_atmosphere_apply"][1] == [c_int, A, POINTER(c_float), c_uint32, c_void_p, c_void_p, c_void_p, c_size_t,
                                                          c_int, c_void_p, c_int, c_void_p]
    assert _params(header, "vr_atmosphere_apply") == [
        "int device", "const vr_atmosphere* atm", "const float translation[3]", "uint32_t scale", "const vr_ray* rays",
        "const vr_hit* hits", "const uint32_t* colors_in", "size_t n", "int inputs_on_device", "uint32_t* colors_out",
        "int outputs_on_device", "void* stream"]
    # every argument of vr_shade_lights_reflect, in its order, then the atmosphere
    assert _capi.SIGNATURES["vr_shade_lights_atmosphere"][1] == _capi.SIGNATURES["vr_shade_lights_reflect"][1] + [A]
    assert _params(header, "vr_shade_lights_atmosphere") == _params(header, "vr_shade_lights_reflect") + ["const vr_atmosphere* atm"]
    assert re.search(r"^#define VR_ATMOS_SKY 1u", header, flags=re.M) and re.search(r"^#define VR_ATMOS_FOG 2u", header, flags=re.M)
    assert (_capi.VR_ATMOS_SKY, _capi.VR_ATMOS_FOG) == (vr.Atmosphere.SKY, vr.Atmosphere.FOG) == (1, 2)
    order = [header.index(s) for s in ("int vr_shade_lights_reflect(", "} vr_atmosphere;", "int vr_atmosphere_default(",
                                       "int vr_atmosphere_apply(", "int vr_shade_lights_atmosphere(", "int vr_camera_rays(")]
    assert order == sorted(order)
    # the struct, field for field
    m = re.search(r"typedef struct \{([^}]*)\} vr_atmosphere;", header)
    fields = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.sub(r"\s+", " ", fields).strip() == ("float zenith[3], horizon[3], nadir[3]; float up[3]; float fog_color[3]; "
                                                  "float fog_start, fog_end; uint32_t flags; uint32_t reserved;")
    assert [f[0] for f in _capi.VrAtmosphere._fields_] == ["zenith", "horizon", "nadir", "up", "fog_color", "fog_start", "fog_end",
                                                           "flags", "reserved"]
    assert ctypes.sizeof(_capi.VrAtmosphere) == 76 and _capi.VrAtmosphere.flags.offset == 68
    # the header states the arithmetic
    block = header[header.index("} vr_atmosphere;"):header.index("int vr_camera_rays(")]
    for word in ("q256", "lerp256", "sqrtf", "fabsf", ">> 8", "fog_end - fog_start", "linear", "per leg", "f2u"):
        assert word in block, word
    for fn in (vr.shade_lights, vr.DeviceScene.shade_lights, vr.render_lights):
        p = inspect.signature(fn).parameters
        assert "atmosphere" in p and p["atmosphere"].default is None, fn
    assert list(inspect.signature(vr.atmosphere_apply).parameters) == ["rays", "hits", "colors", "info", "atmosphere", "device", "stream"]
    mirror = _read("include", "vr.hpp")
    assert "vr_atmosphere_apply(" in mirror and re.search(r"std::vector<uint32_t> atmosphereApply\(", mirror)
    assert "vr_shade_lights_atmosphere(" in mirror and re.search(r"std::vector<uint32_t> shadeLightsAtmosphere\(", mirror)


def test_the_default_atmosphere():
    lib = vr.lib()
    raw = _capi.VrAtmosphere()
    ctypes.memset(ctypes.byref(raw), 0xAB, ctypes.sizeof(raw))
    assert lib.vr_atmosphere_default(ctypes.byref(raw)) == 0
    assert tuple(raw.up) == (0.0, 1.0, 0.0) and raw.flags == _capi.VR_ATMOS_SKY and raw.reserved == 0
    colours = [tuple(raw.zenith), tuple(raw.horizon), tuple(raw.nadir)]
    assert len(set(colours)) == 3 and all(0.0 <= c <= 1.0 for col in colours + [tuple(raw.fog_color)] for c in col)
    assert raw.fog_end > raw.fog_start >= 0.0
    assert lib.vr_atmosphere_default(None) == -1 and "vr_atmosphere_default" in _last_error()
    a = vr.atmosphere_default()
    assert isinstance(a, vr.Atmosphere) and bytes(a.raw) == bytes(raw) and a.flags == 1
    b = vr.Atmosphere(zenith=(0.1, 0.2, 0.3), up=(0, 0, 2), fog_start=0.25, fog_end=4.0, flags=3)
    assert np.allclose(tuple(b.raw.zenith), (0.1, 0.2, 0.3)) and tuple(b.raw.up) == (0.0, 0.0, 2.0) and tuple(b.raw.horizon) == tuple(raw.horizon)
    assert (b.raw.fog_start, b.raw.fog_end, b.flags) == (0.25, 4.0, 3)


def test_atmosphere_apply_invalid_arguments_name_vr_atmosphere_apply():
    lib = vr.lib()
    tr = _capi.f3((0.0, 0.0, 0.0))
    atm = vr.atmosphere_default().raw
    rays = np.zeros(4, dtype=vr.RAY_DTYPE)
    hits = np.zeros(4, dtype=vr.HIT_DTYPE)
    cin = np.full(5, 0x00123456, dtype=np.uint32)
    out = np.full(5, 0xABABABAB, dtype=np.uint32)
    r, h, ci, o = (x.ctypes.data_as(c_void_p) for x in (rays, hits, cin, out))

    def call(device=0, a=ctypes.byref(atm), t=tr, rr=r, hh=h, cc=ci, n=1, oo=o, in_dev=0, out_dev=0):
        return lib.vr_atmosphere_apply(device, a, t, 1, rr, hh, cc, n, in_dev, oo, out_dev, None)

    def invalid(rc, word):
        assert rc == -1 and "vr_atmosphere_apply" in _last_error() and word in _last_error(), _last_error()

    invalid(call(a=None), "NULL")
    invalid(call(a=None, n=0), "NULL")
    invalid(call(t=None), "NULL")
    invalid(call(rr=None), "NULL")
    invalid(call(hh=None), "NULL")
    invalid(call(cc=None), "NULL")
    invalid(call(oo=None), "NULL")
    invalid(call(n=1 << 31), "many")
    invalid(call(n=1 << 40), "many")
    invalid(call(device=-1), "device")
    invalid(call(device=64), "device")
    invalid(call(device=64, n=0), "device")
    for flags in (4, 8, 7, 0x80000000, 0xFFFFFFFF):
        bad = vr.Atmosphere(flags=flags).raw
        invalid(call(a=ctypes.byref(bad)), "flags")
        invalid(call(a=ctypes.byref(bad), n=0), "flags")
    for off in (4, 8, 12, 1):
        invalid(call(rr=c_void_p(rays.ctypes.data + off), in_dev=1), "aligned")
        invalid(call(hh=c_void_p(hits.ctypes.data + off), in_dev=1), "aligned")
    for off in (1, 2, 3):
        invalid(call(cc=c_void_p(cin.ctypes.data + off), in_dev=1), "aligned")
        invalid(call(oo=c_void_p(out.ctypes.data + off), out_dev=1), "aligned")
    assert (out == 0xABABABAB).all() and (cin == 0x00123456).all()                # nothing was written
    assert call(rr=None, hh=None, cc=None, oo=None, n=0) == 0 and call(n=0) == 0
    for flags in (0, 1, 2, 3):
        assert call(a=ctypes.byref(vr.Atmosphere(flags=flags).raw), n=0) == 0
    with pytest.raises(TypeError):
        vr.atmosphere_apply(rays, hits, cin[:4], vr.VoxelSceneInfo(), "sky")
    with pytest.raises(ValueError):
        vr.atmosphere_apply(rays, hits, cin, vr.VoxelSceneInfo(), vr.atmosphere_default())
    assert len(vr.atmosphere_apply(rays[:0], hits[:0], cin[:0], vr.VoxelSceneInfo(), vr.atmosphere_default())) == 0


def test_shade_lights_atmosphere_invalid_arguments_name_vr_shade_lights_atmosphere():
    lib = vr.lib()
    tr = _capi.f3((0.0, 0.0, 0.0))
    amb = _capi.f3((0.25, 0.25, 0.25))
    lights = (_capi.VrLighting * 65)(*[vr.setup_constant_values() for _ in range(65)])
    atm = vr.Atmosphere(flags=3).raw
    rays = np.zeros(4, dtype=vr.RAY_DTYPE)
    hits = np.zeros(4, dtype=vr.HIT_DTYPE)
    colors = np.zeros(5, dtype=np.uint32)
    ao = np.zeros(5, dtype=np.uint32)
    r, h, c, a = (x.ctypes.data_as(c_void_p) for x in (rays, hits, colors, ao))
    fake = ctypes.create_string_buffer(256)      # (every check below comes before the scene is looked at)

    def call(s=fake, algo=1, li=lights, nl=2, am=amb, t=tr, rr=r, n=1, cc=c, hh=h, order=0, in_dev=0, out_dev=0, strength=96,
             apply=0, aa=a, k=128, bounces=2, mask=0, value=0, at=ctypes.byref(atm)):
        return lib.vr_shade_lights_atmosphere(s, algo, li, nl, am, t, 1, rr, n, in_dev, cc, hh, out_dev, order, None, strength, apply,
                                              aa, k, bounces, mask, value, at)

    def invalid(rc, word):
        assert rc == -1 and "vr_shade_lights_atmosphere" in _last_error() and word in _last_error(), _last_error()

    # the case of its own, with and without rays, with and without a descent
    for flags in (4, 8, 7, 0x80000000, 0xFFFFFFFF):
        bad = vr.Atmosphere(flags=flags).raw
        invalid(call(at=ctypes.byref(bad)), "flags")
        invalid(call(at=ctypes.byref(bad), n=0), "flags")
        invalid(call(at=ctypes.byref(bad), k=0, bounces=0), "flags")
    # vr_shade_lights_reflect's cases, under this function's name, with an atmosphere and without
    for at in (ctypes.byref(atm), None):
        invalid(call(k=256, at=at), "reflectivity")
        invalid(call(bounces=5, at=at), "VR_MAX_BOUNCES")
        invalid(call(mask=1, value=2, at=at), "mirror_value")
        invalid(call(strength=256, at=at), "ao_strength")
        invalid(call(apply=2, at=at), "ao_apply")
        invalid(call(s=None, at=at), "NULL")
        invalid(call(t=None, at=at), "NULL")
        invalid(call(li=None, at=at), "NULL")
        invalid(call(nl=65, at=at), "VR_MAX_LIGHTS")
        invalid(call(rr=None, at=at), "NULL")
        invalid(call(cc=None, at=at), "NULL")
        invalid(call(n=1 << 31, at=at), "many")
        invalid(call(algo=7, at=at), "algorithm")
        invalid(call(order=3, at=at), "order")
        invalid(call(rr=c_void_p(rays.ctypes.data + 4), in_dev=1, at=at), "aligned")
        invalid(call(hh=c_void_p(hits.ctypes.data + 8), out_dev=1, at=at), "aligned")
        invalid(call(cc=c_void_p(colors.ctypes.data + 2), out_dev=1, at=at), "aligned")
        invalid(call(aa=c_void_p(ao.ctypes.data + 1), out_dev=1, at=at), "aligned")
    assert not hits.tobytes().strip(b"\0") and not colors.any() and not ao.any()     # nothing was written
    # its sibling still answers under its own name
    assert lib.vr_shade_lights_reflect(None, 1, lights, 2, amb, tr, 1, r, 1, 0, c, h, 0, 0, None, 0, 0, None, 1, 1, 0, 0) == -1
    assert "vr_shade_lights_reflect:" in _last_error()
    # n == 0: nothing to do, with every flag combination
    for flags in (0, 1, 2, 3):
        at = ctypes.byref(vr.Atmosphere(flags=flags).raw)
        assert call(rr=None, cc=None, hh=None, aa=None, n=0, at=at) == 0 and call(n=0, k=0, bounces=0, at=at) == 0
    assert call(n=0, at=None) == 0
