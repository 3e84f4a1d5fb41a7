"""The in-flight side of launch_policy (vr_launch_plan.h), deterministically.

A launch plans as "alone" whenever the device's previous launch was on the same stream or has
finished, so every test that renders on one waited-for stream sees the lone-frame policy only:
heaviest-first dispatch, the lone occupancy, 2 crawl records per wave.  What a pipelined
renderer runs -- grid order with a learned lane order bound, the in-flight occupancy, 32
records per crawl wave -- was reached only when two streams happened to overlap.
vr_debug_force_in_flight makes every launch plan as not alone; vr_debug_last_launch and
vr_debug_order_uses prove that it did.  The knob branches of the policy that no test enters
run in children (tests/policy_run.py, case set `knobs`): the knobs are read once per process."""
from __future__ import annotations

import numpy as np
import pytest

import oracle
from tests.helpers import diff_report, oracle_lighting_from, render_learned
from tests.policy_run import Launches, crawl_view_case, fuzz_case, nan_case, run_child

pytestmark = pytest.mark.gpu

vr = pytest.importorskip("voxelraymarcher_amd")
torch = pytest.importorskip("torch")

ALGOS = [vr.RayMarchAlgorithm.ORIGINAL, vr.RayMarchAlgorithm.LONGEST_AXIS]
ZERO = (0.0, 0.0, 0.0)


CASES = ("crawl-y-plane", "crawl-shadow-x", "nan-camera", "fuzz-1000", "fuzz-5000")


def make(name):
    """(case, translation, stores): a primary and a shadow crawl view (cluster store), the
    NaN-camera frame and two fuzz cases (both stores)."""
    from tests import crawl_views as cv
    kind, _, rest = name.partition("-")
    if kind == "crawl":
        view = {v.name: v for v in cv.VIEWS}[rest]
        return crawl_view_case(view), view.translation, (0,)
    if kind == "nan":
        return nan_case(), ZERO, (0, 1)
    c = fuzz_case(int(rest))
    return c[:8], c[8], (0, 1)


@pytest.mark.parametrize("name", CASES)
def test_forced_in_flight_launches_match_the_oracle(name):
    """Under vr_debug_force_in_flight and default knobs, Schedule.AUTO and Occupancy.AUTO: the
    view launched 2 * slots + 2 times (render_learned), every launch the oracle's frame; every
    launch planned alone 0, heavy 0, hi 1 (launch_policy: AUTO occupancy, not alone,
    VR_INFLIGHT_WAVES on) and 32 crawl records per wave; the lane order was bound on at least
    slots + 1 launches and a work order on none -- grid order under a learned lane order, which
    AUTO enters only this way.  Then one counted launch: pixels and algorithmic bytes.
    (Measured on an MI355X: 0.5 s for the first case, 0.4 s for the NaN frame, under 0.1 s each
    for the others.)"""
    (xyz, rgb, cam, ocam, lit, W, H, scale), tr, stores = make(name)
    info = vr.VoxelSceneInfo(tr, scale)
    for store in stores:
        ref = oracle.Scene(xyz, rgb, store)
        scene = vr.create_scene(xyz, rgb, vr.StorageType(store))
        device = scene.info()["device"]
        try:
            vr.debug_force_in_flight(device, True)
            for algo in ALGOS:
                tag = f"{name} {vr.StorageType(store).name} {algo.name}"
                want, obytes = ref.render(int(algo), ocam, oracle_lighting_from(lit), W, H, scale, tr)
                with Launches(device) as log:
                    bad, first, d = render_learned(scene, algo, cam, lit, info, W, H, 0, H, want, None, 0,
                                                   schedule=vr.Schedule.AUTO)
                    assert not bad, f"{tag}: launches {bad} of {d['launches']} differ: " + diff_report(first, want, W)
                    out = torch.full((W * H,), -1, dtype=torch.int32, device=f"cuda:{device}")
                    ctr = torch.zeros(1, dtype=torch.int64, device=out.device)
                    vr.render_ex(scene, algo, cam, lit, info, W, H, out, counter=ctr)
                    torch.cuda.synchronize()
                print(f"{tag}: {log.report()} {d}")
                assert log.n == d["launches"] + 1
                assert list(log.plans) == [(0, 0, 1, 32)], f"{tag}: (alone, heavy, hi, crawl_rpw) seen: {log.plans}"
                assert d["lane_order_uses"] >= d["slots"] + 1, f"{tag}: the lane order was not bound: {d}"
                # (none bound.  One may still be made: a slot that holds work-order buffers from an
                # earlier view gets its order remade with the lane order, vr_launch.cpp launch)
                assert d["work_order_uses"] == 0, f"{tag}: a work order bound under grid order: {d}"
                # (the counted launch: the lane order bound, still no work order)
                assert log.orders[-1][2] == log.orders[-2][2] + 1 and log.orders[-1][3] == log.orders[-2][3], tag
                got = out.cpu().numpy().view(np.uint32)
                assert np.array_equal(got, want), f"{tag} (counted): " + diff_report(got, want, W)
                assert int(ctr.item()) == obytes, f"{tag}: algorithmic bytes: gpu {int(ctr.item())} != oracle {obytes}"
            # off again: the next launch on the waited-for stream plans as a lone frame's
            vr.debug_force_in_flight(device, False)
            vr.render_ex(scene, ALGOS[0], cam, lit, info, W, H, out)
            torch.cuda.synchronize()
            lone = vr.debug_last_launch(device)
            assert (lone["alone"], lone["heavy"], lone["hi"], lone["crawl_rpw"]) == (1, 1, 0, 2), lone
        finally:
            vr.debug_force_in_flight(device, False)
            scene.close()
            ref.close()


def rises(orders, column, start):
    """The launches from `start` on at which the counter `column` did not rise."""
    return [k for k in range(start, len(orders)) if not orders[k][column] > orders[k - 1][column]]


def test_knob_branches():
    """Four children, one at a time (stop rule of test_gpu_crawl_width.py), each rendering fuzz
    seed 1000 (both stores) and the crawl view x-plane through render_learned, frames exact:
      VR_ORDER_REFRESH=1: from the second round of slots on every launch has a lane order and a
        work order bound and makes both anew (remake_due's remake-while-bound branch);
      VR_CRAWL_SKIP=0: no crawl pass is skipped on the fuzz view, which on the hash store
        defers nothing (the last crawl pass reported 0 records: by default its slots skip);
      VR_INFLIGHT_HEAVY=1, forced in flight: not alone and heaviest first, the work order bound
        on at least slots + 1 launches;
      VR_CRAWL_RPW_IN_FLIGHT=5, forced in flight: 5 records per crawl wave on every launch.
    (Measured on an MI355X: 9 s for the four children, nearly all of it the interpreter's
    start.)"""
    failures = []
    for knobs, in_flight in (({"VR_ORDER_REFRESH": 1}, False), ({"VR_CRAWL_SKIP": 0}, False),
                             ({"VR_INFLIGHT_HEAVY": 1}, True), ({"VR_CRAWL_RPW_IN_FLIGHT": 5}, True)):
        rep, stop, seconds = run_child("knobs", knobs, in_flight)
        assert stop is None, f"no child after this one: {stop}"
        assert rep["error"] is None and rep["runs"] and rep["in_flight"] == in_flight, rep["error"]
        print(f"{knobs}: child {seconds:.1f} s; " +
              "; ".join(f"{r['case']} {r['store']} {r['algo']}: {r['plans']} {r['delta']}" for r in rep["runs"]))
        for r in rep["runs"]:
            tag, d, slots = f"{knobs} {r['case']} store {r['store']} {r['algo']}", r["delta"], r["delta"]["slots"]
            orders = [r["before"]] + r["orders"]           # orders[k]: the counters after launch k (1-based)
            plans = {tuple(p[:4]) for p in r["plans"]}
            if r["mismatch"]:
                failures.append(f"{tag}: {r['mismatch']}")
            if {p[0] for p in plans} != {0 if in_flight else 1}:
                failures.append(f"{tag}: alone: {plans}")
            if "VR_ORDER_REFRESH" in knobs:
                # launch slots + 1 comes round to slot 0, which made its orders on that very launch or
                # holds them; from launch slots + 2 on every slot holds orders: bound and remade
                for col, what in ((0, "lane orders made"), (1, "work orders made"), (2, "lane order uses"),
                                  (3, "work order uses")):
                    flat = rises(orders, col, slots + 2)
                    if flat:
                        failures.append(f"{tag}: {what} did not rise at launches {flat}: {orders}")
            if "VR_CRAWL_SKIP" in knobs:
                if d["crawl_skips"] != 0 or r["crawl_not_run"] != 0:
                    failures.append(f"{tag}: crawl passes skipped: {d}, {r['crawl_not_run']}")
                if r["case"].startswith("fuzz") and r["store"] == 1 and r["records"] != 0:
                    failures.append(f"{tag}: the fuzz view deferred {r['records']} records: no skip to turn off")
            if "VR_INFLIGHT_HEAVY" in knobs:
                if {p[1] for p in plans} != {1} or d["work_order_uses"] < slots + 1:
                    failures.append(f"{tag}: heaviest first in flight: {plans} {d}")
            if "VR_CRAWL_RPW_IN_FLIGHT" in knobs:
                if {p[3] for p in plans} != {5}:
                    failures.append(f"{tag}: crawl records per wave: {plans}")
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:40])
