"""CPU tests of the lane order's test hooks (include/vr.h vr_debug_capture_lane_order,
vr_debug_lane_order): host bookkeeping only, no HIP call."""
from __future__ import annotations

import pytest

vr = pytest.importorskip("voxelraymarcher_amd")


def test_lane_order_hooks_check_device_index():
    vr.debug_capture_lane_order(63)
    for bad in (-1, 64):
        with pytest.raises(vr.VrError):
            vr.debug_capture_lane_order(bad)
        with pytest.raises(vr.VrError):
            vr.debug_lane_order(bad)


def test_lane_order_read_without_capture_is_an_error():
    # arming the capture drops an earlier one: nothing to read until a launch has made an order
    vr.debug_capture_lane_order(62)
    with pytest.raises(vr.VrError):
        vr.debug_lane_order(62)
