"""CPU tests of vr_trace and vr_camera_rays at the C ABI (no device): the symbols are exported and
bound, vr_ray is 32 bytes in every mirror, the TraceOrder values are the header's, and the
argument checks that come before any device work fail with VR_E_INVALID, a message that names
the function, and the output buffer untouched."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np

import voxelraymarcher_amd as vr
from tests import trace_ref
from voxelraymarcher_amd import _capi


def _last_error() -> str:
    return vr.lib().vr_last_error().decode()


def _read(*parts) -> str:
    return open(os.path.join(os.path.dirname(_capi.HERE), *parts)).read()


def test_symbols_and_records():
    lib = vr.lib()
    for name in ("vr_trace", "vr_camera_rays"):
        assert name in _capi.SIGNATURES and getattr(lib, name).argtypes == _capi.SIGNATURES[name][1]
    assert ctypes.sizeof(_capi.VrRay) == 32 and vr.RAY_DTYPE.itemsize == 32
    assert vr.RAY_DTYPE == trace_ref.RAY_DTYPE
    for name, typ in _capi.VrRay._fields_:
        assert vr.RAY_DTYPE.fields[name][1] == getattr(_capi.VrRay, name).offset
        assert vr.RAY_DTYPE.fields[name][0].itemsize == ctypes.sizeof(typ)
    header = _read("include", "vr.h")
    # the header's struct: 3 floats, a word, 3 floats, a word = 32 bytes, and it says so
    m = re.search(r"typedef struct \{([^}]*)\} vr_ray;", header)
    assert m is not None and "32 bytes" in m.group(1)
    fields = re.findall(r"^\s*(float|uint32_t)\s+(\w+)(?:\[(\d)\])?;", m.group(1), flags=re.M)
    assert [(t, n, int(k or 1)) for t, n, k in fields] == [("float", "origin", 3), ("uint32_t", "reserved0", 1),
                                                            ("float", "direction", 3), ("uint32_t", "reserved1", 1)]
    assert 4 * sum(int(k or 1) for _, _, k in fields) == 32
    for name, value in (("AUTO", 0), ("GIVEN", 1), ("COHERENT", 2)):
        assert re.search(rf"VR_TRACE_ORDER_{name} = {value}\b", header)
        assert int(vr.TraceOrder[name]) == value == getattr(_capi, f"VR_TRACE_ORDER_{name}")
    assert callable(vr.trace) and callable(vr.camera_rays) and hasattr(vr.DeviceScene, "trace")
    mirror = _read("include", "vr.hpp")
    assert "vr_trace(" in mirror and "vr_camera_rays(" in mirror


def test_trace_invalid_arguments_name_vr_trace():
    lib = vr.lib()
    tr = _capi.f3((0.0, 0.0, 0.0))
    rays = np.zeros(4, dtype=vr.RAY_DTYPE)
    hits = np.zeros(4, dtype=vr.HIT_DTYPE)
    r, h = rays.ctypes.data_as(ctypes.c_void_p), hits.ctypes.data_as(ctypes.c_void_p)
    # (every check below comes before the scene is looked at: any non-null handle will do)
    fake = ctypes.create_string_buffer(256)

    def call(s=fake, algo=1, t=tr, rr=r, n=1, hh=h, order=0, in_dev=0, out_dev=0):
        return lib.vr_trace(s, algo, t, 1, rr, n, in_dev, hh, out_dev, order, None)

    def invalid(rc, word):
        assert rc == -1 and "vr_trace" in _last_error() and word in _last_error(), _last_error()

    invalid(call(s=None), "NULL")
    invalid(call(t=None), "NULL")
    invalid(call(rr=None), "NULL")
    invalid(call(hh=None), "NULL")
    invalid(call(n=1 << 31), "many")
    invalid(call(n=1 << 40), "many")
    invalid(call(algo=7), "algorithm")
    for order in (3, 7, 0xFFFFFFFF):
        invalid(call(order=order), "order")
    # device arrays must be 16-byte aligned (checked on the pointer alone)
    invalid(call(rr=ctypes.c_void_p(rays.ctypes.data + 4), in_dev=1), "aligned")
    invalid(call(hh=ctypes.c_void_p(hits.ctypes.data + 8), out_dev=1), "aligned")
    assert not hits.tobytes().strip(b"\0")                    # nothing was written
    assert call(rr=None, hh=None, n=0) == 0                   # n == 0: nothing to do, under every order
    for order in (0, 1, 2):
        assert call(n=0, order=order) == 0


def test_camera_rays_invalid_arguments_name_vr_camera_rays():
    lib = vr.lib()
    cam = ctypes.pointer(_capi.VrCamera())
    q = np.zeros(4, dtype=np.uint32)
    rays = np.zeros(4, dtype=vr.RAY_DTYPE)
    p, r = q.ctypes.data_as(ctypes.c_void_p), rays.ctypes.data_as(ctypes.c_void_p)

    def call(device=0, c=cam, W=8, H=8, px=p, py=p, n=1, rr=r, out_dev=0):
        return lib.vr_camera_rays(device, c, W, H, px, py, n, 0, rr, out_dev, None)

    def invalid(rc, word):
        assert rc == -1 and "vr_camera_rays" in _last_error() and word in _last_error(), _last_error()

    invalid(call(c=None), "NULL")
    for a, b, c in ((None, p, r), (p, None, r), (p, p, None)):
        invalid(call(px=a, py=b, rr=c), "NULL")
    for W, H in ((0, 8), (8, 0), (65537, 8), (8, 65537)):
        invalid(call(W=W, H=H), "size")
    invalid(call(n=1 << 31), "many")
    for device in (-1, 64, 1000):
        invalid(call(device=device), "device")
    # device rays must be 16-byte aligned (checked on the pointer alone)
    for off in (4, 8):
        invalid(call(rr=ctypes.c_void_p(rays.ctypes.data + off), out_dev=1), "aligned")
    assert not rays.tobytes().strip(b"\0")                    # nothing was written
    assert call(px=None, py=None, rr=None, n=0) == 0
    assert call(W=65536, H=65536, n=0) == 0
