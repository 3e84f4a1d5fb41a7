"""CPU tests of vr_scene_lookup / vr_scene_paint at the C ABI (no device): the symbols are
exported and bound, VR_VOXEL_ABSENT is VR_VOXEL_REMOVE, and the argument checks that come before
any device work fail with VR_E_INVALID and a message that names the function."""
from __future__ import annotations

import ctypes
import os

import numpy as np

import voxelraymarcher_amd as vr
from voxelraymarcher_amd import _capi


def _last_error() -> str:
    return vr.lib().vr_last_error().decode()


def test_symbols_are_bound():
    lib = vr.lib()
    for name in ("vr_scene_lookup", "vr_scene_paint"):
        assert name in _capi.SIGNATURES and getattr(lib, name).argtypes == _capi.SIGNATURES[name][1]
    assert vr.VOXEL_ABSENT == vr.VOXEL_REMOVE == 0xFFFFFFFF
    header = open(os.path.join(os.path.dirname(_capi.HERE), "include", "vr.h")).read()
    assert "#define VR_VOXEL_ABSENT 0xFFFFFFFFu" in header and "#define VR_VOXEL_REMOVE 0xFFFFFFFFu" in header
    assert "int vr_scene_lookup(const vr_scene* s," in header and "int vr_scene_paint(vr_scene* s," in header
    assert hasattr(vr.DeviceScene, "lookup") and hasattr(vr.DeviceScene, "paint")


def test_null_arguments_are_invalid():
    lib = vr.lib()
    xyz = np.zeros(3, dtype=np.int32)
    rgb = np.zeros(1, dtype=np.uint32)
    px, pc = xyz.ctypes.data_as(ctypes.c_void_p), rgb.ctypes.data_as(ctypes.c_void_p)
    absent = ctypes.c_size_t(77)
    assert lib.vr_scene_lookup(None, px, 1, 0, pc, 0, None) == -1
    assert "NULL" in _last_error() and "vr_scene_lookup" in _last_error()
    assert lib.vr_scene_paint(None, px, pc, 1, 0, None, ctypes.byref(absent)) == -1
    assert "NULL" in _last_error() and "vr_scene_paint" in _last_error()
    # (the array checks come before the scene is looked at: any non-null handle will do)
    fake = ctypes.create_string_buffer(256)
    for a, b in ((None, pc), (px, None), (None, None)):
        assert lib.vr_scene_lookup(fake, a, 1, 0, b, 0, None) == -1
        assert "NULL" in _last_error() and "vr_scene_lookup" in _last_error()
        assert lib.vr_scene_paint(fake, a, b, 1, 0, None, None) == -1
        assert "NULL" in _last_error() and "vr_scene_paint" in _last_error()
    # n >= 2^31
    assert lib.vr_scene_lookup(fake, px, 1 << 31, 0, pc, 0, None) == -1
    assert "too many" in _last_error() and "vr_scene_lookup" in _last_error()
    assert lib.vr_scene_paint(fake, px, pc, 1 << 31, 0, None, None) == -1
    assert "too many" in _last_error() and "vr_scene_paint" in _last_error()
    # n == 0: nothing to do, with or without arrays
    assert lib.vr_scene_lookup(fake, None, 0, 0, None, 0, None) == 0
    assert lib.vr_scene_lookup(fake, px, 0, 1, pc, 1, None) == 0
    assert lib.vr_scene_paint(fake, None, None, 0, 0, None, None) == 0
    assert lib.vr_scene_paint(fake, px, pc, 0, 0, None, ctypes.byref(absent)) == 0 and absent.value == 0
