"""CPU tests of vr_scene_edit / vr_scene_voxels at the C ABI (no device): the symbols are
exported and bound, and the argument checks that come before any device work fail with
VR_E_INVALID and a message."""
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
    for name in ("vr_scene_edit", "vr_scene_voxels"):
        assert name in _capi.SIGNATURES and getattr(lib, name).argtypes == _capi.SIGNATURES[name][1]
    assert vr.VOXEL_REMOVE == 0xFFFFFFFF
    header = os.path.join(os.path.dirname(_capi.HERE), "include", "vr.h")
    assert "#define VR_VOXEL_REMOVE 0xFFFFFFFFu" in open(header).read()
    assert hasattr(vr.DeviceScene, "edit") and hasattr(vr.DeviceScene, "voxels")


def test_null_arguments_are_invalid():
    lib = vr.lib()
    xyz = np.zeros(3, dtype=np.int32)
    rgb = np.zeros(1, dtype=np.uint32)
    px, pc = xyz.ctypes.data_as(ctypes.c_void_p), rgb.ctypes.data_as(ctypes.c_void_p)
    assert lib.vr_scene_edit(None, px, pc, 1, 0, None) == -1
    assert "NULL" in _last_error() and "vr_scene_edit" in _last_error()
    # (the array checks come before the scene is looked at: any non-null handle will do)
    fake = ctypes.create_string_buffer(256)
    for a, b in ((None, pc), (px, None), (None, None)):
        assert lib.vr_scene_edit(fake, a, b, 1, 0, None) == -1
        assert "NULL" in _last_error()
    assert lib.vr_scene_edit(fake, None, None, 0, 0, None) == 0      # n == 0: nothing to do
    n = ctypes.c_size_t(77)
    assert lib.vr_scene_voxels(None, None, None, 0, 0, None, ctypes.byref(n)) == -1
    assert "NULL" in _last_error() and "vr_scene_voxels" in _last_error()
    assert lib.vr_scene_voxels(fake, None, None, 0, 0, None, None) == -1
