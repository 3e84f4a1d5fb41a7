"""Renders under learned lane and work orders against the oracle, where check_frame
(tests/test_gpu_parity.py) cannot reach: odd row ranges, explicit schedules, each rank's
buffer of a tile deal and of row bands, and frames in flight on two streams.

Once a view has been launched more than a ring's worth of times, every tile-pass wave renders
another set of pixels than on the first render (vr_march.hip lane_pixel), the tile groups run
in another order and the crawl pass may be skipped.  The walk takes wave-wide decisions
(ballots over walk_ok and over the fast divisions' checks, one loop per sign pattern present
in the wave), so "an order never changes a pixel" is a property to test, not one that holds by
construction.  Every case is bit-exact against the oracle, launches the view 2 * slots + 2
times (tests/helpers.py render_learned) and asserts from vr_debug_order_uses that the learned
path really ran and that the frame holds a whole lane block."""
from __future__ import annotations

import numpy as np
import pytest

import oracle
from tests.fuzz_cases import make_case, make_wide_case
from tests.helpers import (diff_report, full_lane_blocks, oracle_camera_from, oracle_lighting_from,
                           render_learned)

pytestmark = pytest.mark.gpu

vr = pytest.importorskip("voxelraymarcher_amd")
torch = pytest.importorskip("torch")

STORES = [vr.StorageType.VOXEL_CLUSTER_STORE, vr.StorageType.HASH_TABLE]
ALGOS = [vr.RayMarchAlgorithm.ORIGINAL, vr.RayMarchAlgorithm.LONGEST_AXIS]
# fuzz cases (tests/fuzz_cases.py) with H >= 48; between them point lights, shadows off, scales
# 2, 3, 4 and 7, axis views, zero-component and equal-component lights
SEEDS = [1000, 1003, 1004, 1008, 1013, 1017, 1020, 1026, 1029, 1032, 1033, 1038, 1039, 1042, 1043, 1052,
         5002, 5004, 5006, 5009, 5010, 5011, 5012, 5017]
DEAL_SEEDS = [1000, 1017, 1038, 5004]


class View:
    """One fuzz case: its camera, lights and transform, and per store the GPU and oracle scenes."""

    def __init__(self, seed):
        c = make_wide_case(seed) if seed >= 5000 else make_case(seed)
        self.c, self.W, self.H = c, c.W, c.H
        self.cam = vr.Camera(c.eye, c.look_at, c.up, c.fov, c.aspect)
        self.lit = vr.setup_constant_values(use_shadows=c.shadows, use_point_light=c.point,
                                            light_position=c.light_pos, light_direction=c.light_dir,
                                            light_color=c.light_color)
        self.info = vr.VoxelSceneInfo(c.translation, c.scale)

    def scenes(self):
        for store in STORES:
            ref = oracle.Scene(self.c.xyz, self.c.rgb, int(store))
            gpu = vr.create_scene(self.c.xyz, self.c.rgb, store)
            yield store, gpu, ref
            gpu.close()
            ref.close()

    def want(self, ref, algo, row_begin=0, row_end=None):
        row_end = self.H if row_end is None else row_end
        return ref.render(int(algo), oracle_camera_from(self.cam), oracle_lighting_from(self.lit), self.W, self.H,
                          self.c.scale, self.c.translation, row_begin, row_end)[0]


@pytest.mark.parametrize("seed", SEEDS)
def test_odd_row_ranges(seed):
    """Rows [1 + seed % 7, H - seed % 5): at least 37 rows -- one whole row of lane blocks --
    that never begin on a multiple of 8, against the oracle's same rows."""
    v = View(seed)
    rb, re = 1 + seed % 7, v.H - seed % 5
    assert re - rb >= 37 and rb % 8 != 0
    for store, gpu, ref in v.scenes():
        for algo in ALGOS:
            want = v.want(ref, algo, rb, re)
            bad, first, d = render_learned(gpu, algo, v.cam, v.lit, v.info, v.W, v.H, rb, re, want, None, 0)
            tag = f"seed {seed} {store.name} {algo.name} rows [{rb}, {re})"
            assert not bad, f"{tag}: launches {bad} differ: " + diff_report(first, want, v.W, rb)
            assert full_lane_blocks(v.W, re - rb, d["lane_block"]) >= 1, tag
            assert d["lane_order_uses"] >= d["slots"] + 1, (tag, d)
            assert d["work_order_uses"] >= d["slots"] + 1, (tag, d)


@pytest.mark.parametrize("schedule", [vr.Schedule.GRID, vr.Schedule.HEAVIEST_FIRST], ids=lambda s: s.name)
@pytest.mark.parametrize("seed", SEEDS[:8])
def test_explicit_schedules(seed, schedule):
    """Full frames under an explicit schedule: GRID binds the lane order and never a work
    order, HEAVIEST_FIRST binds both."""
    v = View(seed)
    for store, gpu, ref in v.scenes():
        for algo in ALGOS:
            want = v.want(ref, algo)
            bad, first, d = render_learned(gpu, algo, v.cam, v.lit, v.info, v.W, v.H, 0, v.H, want, None, 0,
                                           schedule=schedule)
            tag = f"seed {seed} {store.name} {algo.name} {schedule.name}"
            assert not bad, f"{tag}: launches {bad} differ: " + diff_report(first, want, v.W)
            assert full_lane_blocks(v.W, v.H, d["lane_block"]) >= 1, tag
            assert d["lane_order_uses"] >= d["slots"] + 1, (tag, d)
            if schedule == vr.Schedule.GRID:
                assert d["work_order_uses"] == 0, (tag, d)
            else:
                assert d["work_order_uses"] >= d["slots"] + 1, (tag, d)


@pytest.mark.parametrize("seed", DEAL_SEEDS)
def test_tile_deal_and_bands(seed):
    """Each rank's buffer of a 3-rank 16x16 tile deal and of 2-rank 8-row bands: every one of
    the launches equals the rank's first render, and the last renders, put together on the
    host, are the oracle's frame.  The lane blocks live in the rank's local buffer
    coordinates here, and a block's pixels may lie past the frame."""
    from voxelraymarcher_amd.tiles import assemble_bands, assemble_tiles
    v = View(seed)
    W, H = v.W, v.H
    deals = [("tiles", dict(band_rows=16, tile_cols=16, nranks=3), vr.tile_buffer_words(W, H, 16, 16, 3)),
             ("bands", dict(band_rows=8, nranks=2), vr.band_buffer_words(W, H, 8, 2))]
    for store, gpu, ref in v.scenes():
        for algo in ALGOS:
            want = v.want(ref, algo)
            for name, deal, words in deals:
                R = deal["nranks"]
                parts = torch.empty((R, words), dtype=torch.int32, device="cuda")
                for r in range(R):
                    tag = f"seed {seed} {store.name} {algo.name} {name} rank {r}"
                    first = torch.full((words,), -1, dtype=torch.int32, device="cuda")
                    vr.render_ex(gpu, algo, v.cam, v.lit, v.info, W, H, first, rank=r, **deal)
                    torch.cuda.synchronize()
                    bad, frame, d = render_learned(gpu, algo, v.cam, v.lit, v.info, W, H, 0, H, first, None, 0,
                                                   out=parts[r], rank=r, **deal)
                    assert not bad, f"{tag}: launches {bad} differ from the rank's first render"
                    assert d["lane_order_uses"] >= d["slots"] + 1, (tag, d)
                    assert d["work_order_uses"] >= d["slots"] + 1, (tag, d)
                if name == "tiles":
                    img = assemble_tiles(parts.cpu(), W, H, 16, 16)
                else:
                    img = assemble_bands(parts, W, H, 8).cpu()
                img = img.numpy().view(np.uint32).reshape(-1)
                assert np.array_equal(img, want), f"seed {seed} {store.name} {algo.name} {name}: " + \
                    diff_report(img, want, W)


@pytest.mark.parametrize("seed", DEAL_SEEDS)
def test_frames_in_flight(seed):
    """The launches issued alternately on two streams into a buffer each, waited for once at the
    end: every buffer is the oracle's frame.  Which policy a launch got (alone: heaviest
    first; with another stream's launch running: grid order, the in-flight occupancy) depends
    on timing and is not asserted -- only the pixels are."""
    v = View(seed)
    W, H = v.W, v.H
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for store, gpu, ref in v.scenes():
        device = gpu.info()["device"]
        n = 2 * vr.debug_order_uses(device)["slots"] + 2
        for algo in ALGOS:
            want = v.want(ref, algo)
            want_t = torch.from_numpy(want.view(np.int32)).cuda()
            bufs = torch.full((n, W * H), -1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            before = vr.debug_order_uses(device)
            for k in range(n):
                vr.render_ex(gpu, algo, v.cam, v.lit, v.info, W, H, bufs[k], stream=streams[k % 2])
            torch.cuda.synchronize()
            after = vr.debug_order_uses(device)
            bad = [k for k in range(n) if not torch.equal(bufs[k], want_t)]
            tag = f"seed {seed} {store.name} {algo.name}"
            assert not bad, f"{tag}: launches {bad} differ: " + \
                diff_report(bufs[bad[0]].cpu().numpy().view(np.uint32), want, W)
            assert after["launches"] - before["launches"] == n
            # The count does not hang on timing (the device lock orders the launches): the view is new,
            # so launch 1 does not repeat it; launches 2 .. slots + 1 repeat it on `slots` distinct slots
            # and each makes its slot's lane order; launches slots + 2 .. 2 slots + 2 find one bound --
            # slots + 1 of them, every slot at least once.
            assert after["lane_order_uses"] - before["lane_order_uses"] >= after["slots"] + 1, tag
