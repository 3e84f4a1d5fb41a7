"""The learned orders' inputs and outputs against a model (tests/order_model.py).  No order ever
changes a pixel, so the parity suite cannot see this data: an order that is a valid permutation
but not heaviest first renders the oracle's frame.  Here

(a) perm_kernel runs on directed walk lengths (vr_debug_lane_order_from): the lane order of every
    full block and every wave's cost word equal the model's;
(b) order_kernel runs on directed costs (vr_debug_work_order_from): a permutation of the grid,
    heaviest class first;
(c) a real launch's captured walk lengths (KView::pcost) equal the oracle's per-pixel primary
    and shadow iteration counts, and the lane order, the costs and the work order that launch
    made from them are the model's;
(d) the same on a view whose tile pass defers pixels to the crawl pass: a deferred pixel's
    walking half is stored as 0xFFFF.

Shapes are what the library reports, so the tests hold for any VR_LANE_BLOCK* / VR_LANE_SEAT
build."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import oracle
from tests import order_cases, order_model
from tests.crawl_views import ASPECT, SCENES, UP, VIEWS
from tests.crawl_views import H as CRAWL_H
from tests.crawl_views import W as CRAWL_W

pytestmark = pytest.mark.gpu

vr = pytest.importorskip("voxelraymarcher_amd")

UNWRITTEN = 0xFFFFFFFF          # the hooks fill their outputs with 0xFF bytes before the kernel runs
FRAME_IDS = ["one-block", "3x2-blocks-and-a-cut-row", "cut-right", "one-pixel-past", "8x8", "1x1"]
LAUNCHES = 40                   # past two uses of each of the ring's 16 slots, as tests/test_gpu_lane_seat.py
TILE_BUDGET = 4096              # vr::kTileBudget: a tile-pass walk past it is the crawl pass's


def lane_block():
    return vr.debug_order_uses(torch.cuda.current_device())["lane_block"]


# ---------------------------------------------------------------- (a) perm_kernel, directed
@pytest.mark.parametrize("pattern", list(order_cases.PCOST_PATTERNS))
@pytest.mark.parametrize("frame", range(len(FRAME_IDS)), ids=FRAME_IDS)
def test_perm_kernel_matches_model(frame, pattern):
    X, Y = lane_block()
    LW, rows = order_cases.frames(X, Y)[frame]
    pcost = order_cases.pcost(pattern, LW, rows, X, Y)
    info, perm, cost = vr.debug_lane_order_from(pcost, torch.cuda.current_device())
    assert (info["LW"], info["rows"], info["block_x"], info["block_y"]) == (LW, rows, X, Y)
    want_perm, want_cost = order_model.lane_order(pcost, LW, rows, info)
    assert (info["gy"], info["gx"], 2) == want_cost.shape == cost.shape
    assert perm.shape == want_perm.shape
    full = want_perm[:, 0] != order_model.UNSPECIFIED
    # keys are distinct, so the deal of a full block is unique
    bad = np.argwhere(perm[full].astype(np.int32) != want_perm[full])
    assert len(bad) == 0, (f"{len(bad)} perm entries differ, first (full block, entry) {bad[0].tolist()}: "
                           f"{int(perm[full][tuple(bad[0])])} for {int(want_perm[full][tuple(bad[0])])}")
    if pattern == "zero" and info["seat"] == 0:
        assert np.array_equal(perm[full].astype(np.int64), np.tile(np.arange(X * Y - 1, -1, -1), (int(full.sum()), 1)))
    # (a cut block's entries are unspecified; the kernel writes none, so the hook's fill is left)
    assert np.all(perm[~full] == np.iinfo(perm.dtype).max)
    assert not np.any(cost == UNWRITTEN), f"cost words left unwritten at (row, column, wave) {np.argwhere(cost == UNWRITTEN)[:4].tolist()}"
    bad = np.argwhere(cost != want_cost)
    assert len(bad) == 0, (f"{len(bad)} cost words differ, first (row, column, wave) {bad[0].tolist()}: "
                           f"{int(cost[tuple(bad[0])])} for {int(want_cost[tuple(bad[0])])}")


# ---------------------------------------------------------------- (b) order_kernel, directed
@pytest.mark.parametrize("pattern", list(order_cases.COST_PATTERNS))
@pytest.mark.parametrize("grid", order_cases.GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_order_kernel_sorts_by_class(grid, pattern):
    gx, gy = grid
    cost = order_cases.cost(pattern, gx, gy)
    order = vr.debug_work_order_from(cost, gx, torch.cuda.current_device())
    assert order.shape == (gx * gy,)
    assert not np.any(order == UNWRITTEN), f"entries left unwritten: {np.flatnonzero(order == UNWRITTEN)[:8].tolist()}"
    order_model.check_work_order(order, cost, gx, gy)


# ---------------------------------------------------------------- (c), (d) what a real launch records and makes
def clamped_pair(iters):
    """The oracle's (primary, shadow) iteration counts as march_kernel stores them."""
    it = np.minimum(iters, 0xFFFF).astype(np.uint32)
    return it[..., 0] << np.uint32(16) | it[..., 1]


def capture_launches(scene, algo, cam, lit, info, W, H):
    """LAUNCHES renders of one view on one stream with the lane order's capture armed: ->
    (the first frame, which every later one equals; the crawl pass's record count read after the
    launch that made the capture)."""
    dev = torch.cuda.current_device()
    vr.forget_orders(dev)
    vr.debug_capture_lane_order(dev)
    first, records = None, None
    for i in range(LAUNCHES):
        out = torch.full((W * H,), -1, dtype=torch.int32, device="cuda")
        vr.run_raymarching_kernel(scene, algo, cam, lit, info, W, H, out)
        torch.cuda.synchronize()
        if first is None:
            first = out.clone()
        assert torch.equal(out, first), (W, H, i)
        if records is None and captured(dev):
            records = vr.debug_last_launch(dev)["records"]
    assert records is not None, "no launch made a lane order"
    return first.cpu().numpy().view(np.uint32), records


def captured(dev) -> bool:
    try:
        vr.debug_lane_order(dev)
    except vr.VrError:
        return False
    return True


def check_captured_orders(W, H, want_pcost=None):
    """The captured launch's lane order, costs and work order against the model, from the walk
    lengths it captured.  -> (info, pcost)."""
    dev = torch.cuda.current_device()
    info, pcost, perm = vr.debug_lane_order(dev)
    cost, order = vr.debug_work_order(dev)
    assert (info["LW"], info["rows"]) == (W, H)
    if want_pcost is not None:
        bad = np.argwhere(pcost != want_pcost)
        assert len(bad) == 0, (f"{len(bad)} of {W * H} pixels' walk lengths differ from the oracle's, first (row, column) "
                               f"{bad[0].tolist()}: {int(pcost[tuple(bad[0])]):#010x} for {int(want_pcost[tuple(bad[0])]):#010x}")
    want_perm, want_cost = order_model.lane_order(pcost, W, H, info)
    full = want_perm[:, 0] != order_model.UNSPECIFIED
    assert perm.shape == want_perm.shape
    assert np.array_equal(perm[full].astype(np.int32), want_perm[full]), np.argwhere(perm[full] != want_perm[full])[:4].tolist()
    assert cost.shape == want_cost.shape
    assert np.array_equal(cost, want_cost), np.argwhere(cost != want_cost)[:4].tolist()
    order_model.check_work_order(order, cost, info["gx"], info["gy"])
    return info, pcost


@pytest.fixture(scope="module")
def c1():
    """C1's voxels, and per store the GPU scene and the oracle's, built once."""
    cfg = vr.CONFIGS["C1"]
    xyz, rgb = cfg.voxels()
    made = {}

    def get(store):
        if store not in made:
            st = vr.parse_storage(store)
            made[store] = (vr.create_scene(xyz, rgb, st), oracle.Scene(xyz, rgb, int(st)))
        return cfg, made[store]
    yield get
    for g, o in made.values():
        g.close()
        o.close()


@pytest.mark.parametrize("size", [(48, 40), (48, 72), (17, 33)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("algo", [vr.RayMarchAlgorithm.ORIGINAL, vr.RayMarchAlgorithm.LONGEST_AXIS], ids=lambda a: a.name)
@pytest.mark.parametrize("store", ["vcs", "hashtable"])
def test_captured_launch_matches_oracle_and_model(c1, store, algo, size):
    """C1 at its own scale.  The oracle's longest walk on these views is 135 iterations and 543 to
    3263 pixels have a shadow walk (asserted below), so nothing defers, nothing saturates and
    both halves are exercised: pcost must be the oracle's per-pixel (primary, shadow) iteration
    counts exactly, at every pixel."""
    W, H = size
    cfg, (scene, ref) = c1(store)
    assert cfg.scale == 12
    cam, lit = vr.Camera.reference(W, H), vr.setup_constant_values()
    got, _ = capture_launches(scene, algo, cam, lit, vr.VoxelSceneInfo((0.0, 0.0, 0.0), cfg.scale), W, H)
    ocam, olit = oracle.reference_camera(W, H), oracle.lighting()
    want, _ = ref.render(int(algo), ocam, olit, W, H, cfg.scale)
    assert np.array_equal(got, np.asarray(want).reshape(-1)), (store, W, H)
    iters = ref.pixel_stats(int(algo), ocam, olit, W, H, cfg.scale)[..., 6]
    assert iters.shape == (H, W, 2) and 0 < int(iters.max()) < TILE_BUDGET
    assert np.count_nonzero(iters[..., 0]) >= W * H // 2 and np.count_nonzero(iters[..., 1]) >= 500
    check_captured_orders(W, H, clamped_pair(iters))


def crawl_view(name):
    """(view, GPU camera and lights, oracle camera and lights) of a tests/crawl_views.py view."""
    from tests.test_gpu_crawl_views import oracle_view
    view = next(v for v in VIEWS if v.name == name)
    cam = vr.Camera(view.world(view.eye), view.world(view.look_at), UP, view.fov, ASPECT)
    lit = vr.setup_constant_values(use_point_light=view.point, light_position=view.light_pos, light_direction=view.light_dir)
    return view, cam, lit, oracle_view(view)


@pytest.mark.parametrize("algo", [vr.RayMarchAlgorithm.ORIGINAL, vr.RayMarchAlgorithm.LONGEST_AXIS], ids=lambda a: a.name)
@pytest.mark.parametrize("name", ["y-plane", "shadow-x"])
def test_captured_launch_with_deferred_pixels(name, algo):
    """A pixel the tile pass hands to the crawl pass leaves the tile pass early and stores 0xFFFF in
    the half that was walking, so it ranks as the heaviest of its block.  The tile pass defers
    for two reasons only (vr_walk.h, vr_march.hip shade): a cluster-skip crawl -- the original
    walk writes a crawl record and leaves kDeferredIters in the walker, the longest-axis walk
    hands the pixel over to be walked from its start -- and a walk past the tile budget.  So:
    every pixel is the clamped oracle pair or has 0xFFFF in a half; those that are not the
    oracle pair are at most the crawl pass's record count, which is at most the pixels with a
    cluster skip or a walk of the tile budget; and the walks of >= 65 536 iterations hold
    0xFFFF.  (Before march_kernel saturated every deferred pixel the longest-axis cases failed:
    the 48 crawling pixels of "y-plane" stored 0x00090000, the count at which they gave up.)"""
    view, cam, lit, (ocam, olit) = crawl_view(name)
    W, H = CRAWL_W, CRAWL_H
    xyz, rgb = SCENES[view.scene]()
    scene = vr.create_scene(xyz, rgb, vr.StorageType.VOXEL_CLUSTER_STORE)
    ref = oracle.Scene(xyz, rgb, oracle.STORE_VCS)
    try:
        got, records = capture_launches(scene, algo, cam, lit, vr.VoxelSceneInfo(view.translation, view.scale), W, H)
        want, _ = ref.render(int(algo), ocam, olit, W, H, view.scale, view.translation)
        assert np.array_equal(got, np.asarray(want).reshape(-1))
        st = ref.pixel_stats(int(algo), ocam, olit, W, H, view.scale, view.translation)
    finally:
        scene.close()
        ref.close()
    iters = st[..., 6]
    want_pcost = clamped_pair(iters)
    _, pcost = check_captured_orders(W, H)
    differs = pcost != want_pcost
    saturated = ((pcost >> 16) == 0xFFFF) | ((pcost & 0xFFFF) == 0xFFFF)
    can_defer = np.any(st[..., 2] > 0, axis=-1) | np.any(iters >= TILE_BUDGET, axis=-1)
    half = 1 if view.shadow else 0
    long_walk = iters[..., half] >= 65536
    print(f"{name} {algo.name}: {int(differs.sum())} pixels differ from the oracle pair, {int(saturated.sum())} hold 0xFFFF, "
          f"{records} crawl records, {int(can_defer.sum())} pixels can defer, {int(long_walk.sum())} long walks")
    bad = np.argwhere(differs & ~saturated)
    assert len(bad) == 0, (f"{len(bad)} pixels are neither the oracle's pair nor saturated, first (row, column) {bad[0].tolist()}: "
                           f"{int(pcost[tuple(bad[0])]):#010x} for {int(want_pcost[tuple(bad[0])]):#010x}")
    assert int(differs.sum()) <= records <= int(can_defer.sum())
    assert int(long_walk.sum()) >= (5 if view.shadow else 48)
    stored = (pcost & 0xFFFF) if view.shadow else (pcost >> 16)
    assert np.all(stored[long_walk] == 0xFFFF)
