"""The crawl pass against the oracle at every records-per-wave width.

launch_policy (vr_launch_plan.h) gives a lone frame 2 records per crawl wave, frames in flight
32, and VR_CRAWL_RPW = 1..64 any width for every launch.  Almost every other test renders on one
waited-for stream, so its crawl pass runs at width 2 -- two lanes per wave: nearly nothing of a
wave's shared state (each lane's 64-byte LDS slot of cluster-existence bits, the ballots and
readfirstlane dispatch of the walker) is exercised, and above 32 (vr_march.hip kCrawlMaxRpw) no
lane has a slot at all and every skip step loads from memory: another code path.

The width is a knob read once per process, so each width is one child (tests/policy_run.py,
case set `width`) that proves from vr_debug_last_launch which width its launches really ran."""
from __future__ import annotations

import numpy as np
import pytest

import oracle
from tests.crawl_views import H, LONG_WALK, VIEWS, W
from tests.policy_run import NAN_FRAME, run_child
from tests.test_gpu_crawl_views import ALGO_IDS, ALGOS, oracle_view, voxels

WIDTHS = (1, 2, 3, 31, 32, 33, 64)
LDS_WIDTHS = 32          # vr_march.hip kCrawlMaxRpw: the widths whose lanes have an LDS slot
FIRST_GRID = 64          # workgroups of a process's first crawl pass (no hint yet), 2 waves each
WIDE_VIEWS = ("x-plane", "z-plane")


@pytest.mark.parametrize("algo", ALGOS, ids=ALGO_IDS.get)
@pytest.mark.parametrize("name", WIDE_VIEWS)
def test_wide_views_fill_a_wave_in_the_oracle(name, algo):
    """x-plane and z-plane have more than 64 pixels whose primary walk runs >= LONG_WALK
    iterations (tests/crawl_views.py's docstring: 160 and 96).  Every such walk is past the
    tile pass's budget and therefore deferred, so the count is a lower bound on the crawl
    pass's records: at every width up to 64 some crawl wave is full."""
    view = {v.name: v for v in VIEWS}[name]
    ref = oracle.Scene(*voxels(view.scene), oracle.STORE_VCS)
    cam, lit = oracle_view(view)
    iters = ref.pixel_stats(algo, cam, lit, W, H, view.scale, view.translation)[..., 6]
    n_long = int(np.count_nonzero(iters[..., 0] >= LONG_WALK))
    ref.close()
    print(f"{name} {ALGO_IDS[algo]}: {n_long} primary walks of >= {LONG_WALK} iterations")
    assert n_long > max(WIDTHS)
    assert n_long == {"x-plane": 160, "z-plane": 96}[name]


def key(run):
    return run["case"], run["store"], run["algo"], run["kernel"], run["defer_cap"]


def check_child(w, rep):
    """What one child must prove by itself; returns the failures."""
    bad = []
    for r in rep["runs"]:
        tag = f"width {w} {key(r)}"
        if r["mismatch"]:
            bad.append(f"{tag}: {r['mismatch']}")
        widths = sorted({p[3] for p in r["plans"]} | {r["first"]["crawl_rpw"]})
        if widths != [w]:
            bad.append(f"{tag}: launches ran at widths {widths}")
        # (a view defers the same pixels on every launch: one whose first launch reported
        # records must run its crawl pass every time)
        if r["first"]["records"] and (r["crawl_not_run"] or not r["first"]["crawl_ran"]):
            bad.append(f"{tag}: deferred {r['first']['records']} records, {r['crawl_not_run']} launches without a crawl pass")
    first = rep["runs"][0]
    if w <= 3:
        # the record loop's second trip (i += nwaves * rpw): more records than one trip of the grid takes
        f = first["first"]
        if not (first["case"] == NAN_FRAME and f["crawl_grid"] == FIRST_GRID and f["records"] > FIRST_GRID * 2 * w):
            bad.append(f"width {w}: the first launch did not need a second trip: {key(first)} {f}")
    views = [r["first"]["records"] for r in rep["runs"] if r["case"].startswith("crawl-")]
    if not views or max(views) <= w:
        bad.append(f"width {w}: no crawl view deferred more than {w} records: {views}")
    return bad


def check_stats(reports):
    """stats[0] (crawl iterations fast-forwarded in closed form) and stats[1] (bytes credited
    without a load: 4 per fast-forwarded iteration and per skip step answered from a lane's LDS
    bits) across the children, against the width-2 child's; returns the failures.

    Per run (case, algorithm, kernel): stats[0] equal at every width; stats[1] equal for
    w <= 32; for w in {33, 64} on the crawl views stats[1] strictly smaller under the original
    algorithm and not larger under longest axis.  Per crawl view and kernel, both algorithms
    together (the view's credit): strictly smaller for w in {33, 64}.  The longest-axis walk
    never consults the cluster bits (performVoxelSpaceJump's crawls run without them by design,
    vr_crawl.h crawl_run), so where its walks contain no original-DDA stretch its credit cannot
    depend on the slots: the strict drop of a view is the original algorithm's, and the per-run
    conditions are together stronger than the per-view one.

    Only the runs with the default capacity are compared: with a list of 4 records the tile
    pass's lanes race for its places, the winners are resumed with an LDS slot and every other
    deferred pixel is walked from its start without one, so both figures move from launch to
    launch (y-plane, original, TILE, width 2: 14 195 222 in one process, 14 195 257 in the
    next) -- no property of the width."""
    bad = []
    base = {key(r): r["stats"] for r in reports[2]["runs"]}
    for w, rep in sorted(reports.items()):
        view_credit = {}
        for r in rep["runs"]:
            if r["defer_cap"] != 0:
                continue
            k, s, b = key(r), r["stats"], base.get(key(r))
            if b is None:
                bad.append(f"width {w} {k}: no width-2 run to compare with")
                continue
            if s[0] != b[0]:
                bad.append(f"width {w} {k}: stats[0] {s[0]} != width 2's {b[0]}")
            if w <= LDS_WIDTHS and s[1] != b[1]:
                bad.append(f"width {w} {k}: stats[1] {s[1]} != width 2's {b[1]}")
            if w > LDS_WIDTHS and r["case"].startswith("crawl-"):
                if r["algo"] == "ORIGINAL" and not s[1] < b[1]:
                    bad.append(f"width {w} {k}: stats[1] {s[1]} is not below width 2's {b[1]}")
                if not s[1] <= b[1]:
                    bad.append(f"width {w} {k}: stats[1] {s[1]} is above width 2's {b[1]}")
                c = view_credit.setdefault((r["case"], r["kernel"]), [0, 0, 0])
                c[0], c[1], c[2] = c[0] + s[1], c[1] + b[1], c[2] + 1
        for (case, kernel), (got, was, n) in sorted(view_credit.items()):
            if n != 2 or not got < was:
                bad.append(f"width {w} {case} {kernel}: the view's stats[1] {got} over {n} algorithms is not below "
                           f"width 2's {was}")
        if w > LDS_WIDTHS and len(view_credit) != 2 * len(VIEWS):
            bad.append(f"width {w}: {len(view_credit)} (view, kernel) credits, not {2 * len(VIEWS)}")
    return bad


REPORTS: dict = {}       # width -> its child's report, kept by test_crawl_pass_at_every_width


@pytest.mark.gpu
def test_crawl_pass_at_every_width():
    """One child per width in WIDTHS with VR_CRAWL_RPW=<w>, one at a time; a child that ends
    by a signal, a stop code, an error or at its timeout is the last one started, and the test
    fails with what it left.  Each child renders policy_run's `width` cases -- every crawl view
    through both deferral forms and an overflowing list, the NaN-camera and degenerate-light
    frames on both stores -- against the oracle, pixels and algorithmic bytes, and proves from
    vr_debug_last_launch: every launch ran at width w; every launch of a deferring view ran its
    crawl pass; for w <= 3 the child's first launch (the NaN frame, 64-workgroup grid, 4096
    records) had more records than 128 waves x w, so the record loop made a second trip; some
    crawl view deferred more than w records (x-plane 160, z-plane 96), so some wave was full.

    Measured on an MI355X: a child takes 6-7 s, of which its 80 runs (3040 launches) take
    4.5-4.7 s -- the slowest run, 38 launches of a view whose list overflows, 0.2 s -- and the
    rest is the interpreter's start; the NaN frame's 38 launches take 0.1-0.2 s at every width,
    width 1 included, so no case is dropped from any width.  (The degenerate-light frame defers
    nothing at 96x96: its walks end inside the tile pass's budget, its crawl pass is skipped
    once its slots have seen that.  The records past the budget are the NaN frame's.)"""
    REPORTS.clear()
    failures = []
    for w in WIDTHS:
        rep, stop, seconds = run_child("width", {"VR_CRAWL_RPW": w})
        if rep is not None:
            firsts = sorted({(r["first"]["crawl_rpw"], r["first"]["crawl_grid"], r["first"]["records"])
                             for r in rep["runs"]})
            print(f"width {w}: child {seconds:.1f} s, cases {rep['seconds']} s, {len(rep['runs'])} runs, "
                  f"{sum(r['launches'] for r in rep['runs'])} launches, slowest run "
                  f"{max([r['seconds'] for r in rep['runs']], default=0)} s, NaN frame "
                  f"{[r['seconds'] for r in rep['runs'] if r['case'] == NAN_FRAME]} s; the (crawl_rpw, crawl grid, "
                  f"records) of the runs' first launches: {firsts}")
        assert stop is None, f"no child after width {w}: {stop}"
        assert rep["error"] is None and rep["runs"], rep["error"]
        REPORTS[w] = rep
        failures += check_child(w, rep)
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:40])


@pytest.mark.gpu
def test_stats_across_widths():
    """The stats pairs of test_crawl_pass_at_every_width's children (their JSON lines; no child
    is started here) against the width-2 child's (check_stats): for every w <= 32 both figures
    equal -- the LDS slots were on; for w in {33, 64} stats[0] equal and stats[1], the credit
    without a load, strictly smaller on every crawl view -- no LDS copy answered a skip step.

    stats[0] is equal above 32 because a crawl lane without a slot still runs the crawls'
    closed form across the faces of absent clusters, reading the region's cluster bits from
    memory (vr_walk.h Walker::mem_bits).  Before that, each crossing step went back to the walk
    loop above 32 and fewer iterations were fast-forwarded: x-plane, original, TILE: 63 573 773
    at width 2, 63 567 494 at 33.  stats[1] at width 2 / 33, original algorithm: x-plane
    254 299 784 / 254 269 976, y-plane 56 790 064 / 56 780 292; longest axis: x-plane
    253 327 780 at every width (no walk of it reads the bits), y-plane 45 275 772 /
    45 275 744."""
    assert sorted(REPORTS) == sorted(WIDTHS), "test_crawl_pass_at_every_width did not leave every width's report"
    for w in (2, 33):
        print(f"width {w}: " + "; ".join(f"{key(r)} {r['stats']}" for r in REPORTS[w]["runs"] if r["stats"][0]))
    failures = check_stats(REPORTS)
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:60])
