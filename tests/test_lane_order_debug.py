"""CPU tests of the lane and work orders' test hooks (include/vr.h vr_debug_capture_lane_order,
vr_debug_lane_order, vr_debug_work_order, vr_debug_lane_order_from, vr_debug_work_order_from):
host bookkeeping and argument checks only, no HIP call."""
from __future__ import annotations

import ctypes

import numpy as np
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


def test_work_order_read_checks_device_and_capture():
    for bad in (-1, 64):
        with pytest.raises(vr.VrError):
            vr.debug_work_order(bad)
        assert vr.lib().vr_debug_work_order(bad, None, 0, None, 0) != 0
    vr.debug_capture_lane_order(61)
    with pytest.raises(vr.VrError):
        vr.debug_work_order(61)
    assert vr.lib().vr_debug_work_order(61, None, 0, None, 0) != 0
    assert b"no work order captured" in vr.lib().vr_last_error()


def _lane_from(device, pcost, LW, rows, info, perm, perm_bytes, cost, cost_words):
    ptr = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    return vr.lib().vr_debug_lane_order_from(device, ptr(pcost), LW, rows, info, ptr(perm), perm_bytes, ptr(cost),
                                             cost_words)


def test_lane_order_from_checks_its_arguments():
    """Everything is refused before any device work: this machine has no GPU."""
    LW, rows = 20, 40
    raw = (ctypes.c_uint32 * 8)()
    # the sizes: all three arrays NULL fills info and runs nothing
    assert _lane_from(0, None, LW, rows, raw, None, 0, None, 0) == 0
    info = dict(zip(("LW", "rows", "gx", "gy", "block_x", "block_y", "entry_bytes", "seat"), (int(x) for x in raw)))
    assert (info["LW"], info["rows"], info["gx"], info["gy"]) == (LW, rows, 2, 5)
    assert vr.debug_order_uses(0)["lane_block"] == (info["block_x"], info["block_y"])
    assert info["entry_bytes"] == (1 if info["block_x"] * info["block_y"] == 256 else 2) and info["seat"] in (0, 1)
    blocks = -(-LW // info["block_x"]) * -(-rows // info["block_y"])
    nperm = blocks * info["block_x"] * info["block_y"] * info["entry_bytes"]
    ncost = 2 * info["gx"] * info["gy"]
    pcost = np.zeros((rows, LW), dtype=np.uint32)
    perm, cost = np.zeros(nperm, dtype=np.uint8), np.zeros(ncost, dtype=np.uint32)
    ok = (0, pcost, LW, rows, raw, perm, nperm, cost, ncost)

    def refused(**change):
        names = ("device", "pcost", "LW", "rows", "info", "perm", "perm_bytes", "cost", "cost_words")
        args = dict(zip(names, ok))
        args.update(change)
        assert _lane_from(*(args[n] for n in names)) != 0, change
        return vr.lib().vr_last_error().decode()

    assert "device index" in refused(device=-1)
    assert "device index" in refused(device=64)
    assert "info is NULL" in refused(info=None)
    for name in ("pcost", "perm", "cost"):
        assert "NULL" in refused(**{name: None})
    for name in ("LW", "rows"):
        assert "frame size" in refused(**{name: 0})
        assert "frame size" in refused(**{name: 65537})
    for n in (0, nperm - 1, nperm + 1):
        assert "perm_bytes" in refused(perm_bytes=n)
    for n in (0, ncost - 1, ncost + 1, ncost // 2):
        assert "cost_words" in refused(cost_words=n)
    with pytest.raises(ValueError):
        vr.debug_lane_order_from(np.zeros(8, dtype=np.uint32))
    with pytest.raises(vr.VrError):
        vr.debug_lane_order_from(pcost, 64)


def test_work_order_from_checks_its_arguments():
    cost, order = np.zeros(2 * 6, dtype=np.uint32), np.zeros(6, dtype=np.uint32)
    ptr = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    call = vr.lib().vr_debug_work_order_from
    for device in (-1, 64):
        assert call(device, ptr(cost), 3, 6, ptr(order)) != 0
        assert b"device index" in vr.lib().vr_last_error()
    assert call(0, None, 3, 6, ptr(order)) != 0 and b"NULL" in vr.lib().vr_last_error()
    assert call(0, ptr(cost), 3, 6, None) != 0 and b"NULL" in vr.lib().vr_last_error()
    for columns, groups in ((0, 6), (3, 0), (4, 6), (7, 6), (4097, 4097), (1, 8193)):
        assert call(0, ptr(cost), columns, groups, ptr(order)) != 0, (columns, groups)
        assert b"bad grid" in vr.lib().vr_last_error()
    with pytest.raises(ValueError):
        vr.debug_work_order_from(np.zeros(5, dtype=np.uint32), 1)
    with pytest.raises(vr.VrError):
        vr.debug_work_order_from(cost, 4)              # 6 groups in rows of 4
    with pytest.raises(vr.VrError):
        vr.debug_work_order_from(cost, 3, 64)
