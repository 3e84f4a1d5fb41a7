"""CPU tests of the two launch-policy test hooks of include/vr.h, vr_debug_force_in_flight and
vr_debug_last_launch: host bookkeeping only, no HIP call, so they answer with or without a GPU.
What they report about real launches is tests/test_gpu_in_flight_policy.py's and
tests/test_gpu_crawl_width.py's business."""
from __future__ import annotations

import ctypes

import pytest

import voxelraymarcher_amd as vr


def test_last_launch_of_a_device_that_never_rendered():
    """All eight words are 0 (the caller's buffer is overwritten), the dict has the documented
    keys in the documented order, and reading moves nothing."""
    d = vr.debug_last_launch(60)
    assert list(d) == ["alone", "heavy", "hi", "crawl_rpw", "crawl_grid", "crawl_ran", "records"]
    assert not any(d.values())
    raw = (ctypes.c_uint64 * 8)(*[7] * 8)
    assert vr.lib().vr_debug_last_launch(60, raw) == 0
    assert list(raw) == [0] * 8
    assert vr.debug_last_launch(60) == d


def test_last_launch_argument_errors():
    for bad in (-1, 64):
        with pytest.raises(vr.VrError) as e:
            vr.debug_last_launch(bad)
        assert e.value.code == -1
    assert vr.lib().vr_debug_last_launch(60, None) == -1      # VR_E_INVALID: out is NULL
    assert b"NULL" in vr.lib().vr_last_error()


def test_force_in_flight_is_host_state_only():
    """Valid devices succeed on and off without a GPU and a device that never rendered still
    reports zeros afterwards (the hook changes how launches plan, and there were none)."""
    try:
        for dev in (59, 63):
            vr.debug_force_in_flight(dev, True)
            vr.debug_force_in_flight(dev, True)      # sticky: turning it on twice is no error
            assert not any(vr.debug_last_launch(dev).values())
            assert not any(list(vr.debug_order_uses(dev).values())[:6])
    finally:
        for dev in (59, 63):
            vr.debug_force_in_flight(dev, False)
    for bad in (-1, 64):
        with pytest.raises(vr.VrError) as e:
            vr.debug_force_in_flight(bad, True)
        assert e.value.code == -1
        assert vr.lib().vr_debug_force_in_flight(bad, 0) == -1
