"""CPU tests of the pick reference (tests/pick_ref.py) against the C oracle, so that the
yardstick is proven before tests/test_gpu_pick.py judges the kernel with it: the pixel
recomputed from a record alone is the oracle's shadows-off pixel (under a point light, whose
shading reads every field of the record but the voxel, and under the directional light),
a record is VOXEL exactly where the oracle counts a primary hit, the voxel is stored in the
scene with the record's colour, and never-finishing walks are NEVER."""
from __future__ import annotations

import os

import numpy as np
import pytest

import oracle
from tests import pick_ref, pyref
from tests.crawl_views import ASPECT, H as CH, LONG_WALK, SCENES, UP, VIEWS, W as CW
from tests.helpers import GOLDEN
from tests.test_oracle import nan_camera

LIGHT_POS = (40.0, 90.0, 30.0)
PAIRS = [(s, a) for s in (oracle.STORE_VCS, oracle.STORE_HASHTABLE) for a in (oracle.ALGO_ORIGINAL, oracle.ALGO_LONGESTAXIS)]
PAIR_ID = lambda p: f"{'vcs' if p[0] == 0 else 'hash'}-{'original' if p[1] == 1 else 'longest'}"   # noqa: E731


def voxel_dict(xyz, rgb):
    d = {}
    for p, c in zip(np.asarray(xyz).tolist(), np.asarray(rgb).tolist()):
        d[tuple(p)] = c                       # later duplicates win
    return d


def check_against_oracle(xyz, rgb, store, algo, cam, W, H, scale, translation, px, py, min_hits):
    """The records of pixels (px, py) against the oracle: shading, hit/miss, stored voxel.
    -> (records, iterations)."""
    sc = oracle.Scene(xyz, rgb, store)
    ps = pyref.Scene(xyz, rgb, store)
    stored = voxel_dict(xyz, rgb)
    longest = algo == oracle.ALGO_LONGESTAXIS
    recs, iters = pick_ref.pick_pixels(ps, cam, W, H, px, py, scale, longest, translation)
    status = recs["status"]
    assert np.isin(status, (pick_ref.MISS, pick_ref.VOXEL)).all()
    # the oracle's primary-hit counter, both directions (the converse holds too: a walk that
    # reads a stored colour returns at once, in both restatements)
    hits = sc.pixel_stats(algo, cam, oracle.lighting(use_shadows=False), W, H, scale, translation)[..., 0, 5]
    assert np.array_equal(status == pick_ref.VOXEL, hits[py, px] >= 1)
    assert int(np.count_nonzero(status == pick_ref.VOXEL)) >= min_hits
    for point in (True, False):
        olit = oracle.lighting(use_shadows=False, use_point_light=point, light_position=LIGHT_POS)
        plit = pyref.Lighting(False, point, LIGHT_POS)
        want, _ = sc.render_pixels(algo, cam, olit, W, H, scale, px.astype(np.uint32), py.astype(np.uint32),
                                   translation=translation)
        for i in range(len(px)):
            got = pick_ref.shade(ps, recs[i], plit, translation)
            assert got == int(want[i]), (point, int(px[i]), int(py[i]), hex(got), hex(int(want[i])), recs[i])
    # the walk's own colour (pyref.render_pixel) is the same pixel
    pc = pick_ref.cam_fields(cam)
    plit = pyref.Lighting(False, True, LIGHT_POS)
    for i in range(0, len(px), 7):
        assert pyref.render_pixel(ps, plit, pc, W, H, int(px[i]), int(py[i]), scale, longest,
                                  translation=translation) == pick_ref.shade(ps, recs[i], plit, translation)
    for r in recs[status == pick_ref.VOXEL]:
        assert stored.get(tuple(int(c) for c in r["voxel"])) == int(r["color"]), r
        assert sorted(np.abs(r["normal"]).tolist()) == [0, 0, 1]
        assert not r["reserved"].any()
    for r in recs[status != pick_ref.VOXEL]:
        assert r.tobytes()[4:] == bytes(60)
    sc.close()
    return recs, iters


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_ID)
def test_reference_on_golden_scene(pair):
    store, algo = pair
    d = np.load(os.path.join(GOLDEN, "c1_scene.npz"))
    W = H = 256
    rng = np.random.default_rng(300 + 2 * store + algo)
    px, py = rng.integers(0, W, 150), rng.integers(0, H, 150)
    check_against_oracle(d["xyz"], d["rgb"], store, algo, oracle.reference_camera(W, H), W, H, 12, (0.0, 0.0, 0.0),
                         px, py, min_hits=30)


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_ID)
@pytest.mark.parametrize("name", ["y-plane", "y-plane-scale2"])
def test_reference_on_crawl_views(name, pair):
    """Views whose primary walks crawl for 10^5 iterations and more (tests/crawl_views.py), one of
    them scaled and translated.  Sampled: the hash table's longest-axis walk is slow here."""
    store, algo = pair
    view = {v.name: v for v in VIEWS}[name]
    xyz, rgb = SCENES[view.scene]()
    cam = oracle.camera(view.world(view.eye), view.world(view.look_at), UP, view.fov, ASPECT)
    n = 64 if (store, algo) == (oracle.STORE_HASHTABLE, oracle.ALGO_LONGESTAXIS) else 256
    idx = np.random.default_rng(17).permutation(CW * CH)[:n]
    _, iters = check_against_oracle(xyz, rgb, store, algo, cam, CW, CH, view.scale, view.translation, idx % CW,
                                    idx // CW, min_hits=1)
    if store == oracle.STORE_VCS:                # (the cuckoo store has no cluster skips: no crawls)
        assert int(np.count_nonzero(iters >= LONG_WALK)) >= 3


def test_outside_pixels():
    d = np.load(os.path.join(GOLDEN, "c1_scene.npz"))
    ps = pyref.Scene(d["xyz"], d["rgb"], 0)
    cam = oracle.reference_camera(32, 24)
    for x, y in ((32, 0), (0, 24), (0xFFFFFFFF, 0xFFFFFFFF)):
        r, _, _ = pick_ref.pick_pixel(ps, cam, 32, 24, x, y, 12, False)
        assert int(r["status"]) == pick_ref.OUTSIDE and r.tobytes()[4:] == bytes(60)


def test_never_finishing_walks_are_never():
    """The NaN camera of tests/test_oracle.py at 4x4, scale 12.  A pick walks the primary ray
    only, so it is NEVER exactly where the oracle's frame WITHOUT shadows counts only the pixel
    write (4 bytes): both stores' original walks.  In the frame with shadows every NEVER pixel
    counts 4 bytes too, but not the other way round: the cluster store's longest-axis primary
    walk ends in a voxel (with a NaN hit point) and it is the shadow walk from there that never
    finishes -- a VOXEL record, as for the hash table's longest-axis walk, whose walks all end."""
    d = np.load(os.path.join(GOLDEN, "c1_scene.npz"))
    cam = nan_camera()
    px, py = np.arange(16) % 4, np.arange(16) // 4
    upx, upy = px.astype(np.uint32), py.astype(np.uint32)
    seen = {}
    for store, algo in PAIRS:
        sc = oracle.Scene(d["xyz"], d["rgb"], store)
        ps = pyref.Scene(d["xyz"], d["rgb"], store)
        _, nb_primary = sc.render_pixels(algo, cam, oracle.lighting(use_shadows=False), 4, 4, 12, upx, upy)
        _, nb_shadows = sc.render_pixels(algo, cam, oracle.lighting(), 4, 4, 12, upx, upy)
        recs, _ = pick_ref.pick_pixels(ps, cam, 4, 4, px, py, 12, algo == oracle.ALGO_LONGESTAXIS)
        never = recs["status"] == pick_ref.NEVER
        assert np.array_equal(never, np.asarray(nb_primary) == 4), (store, algo)
        assert (np.asarray(nb_shadows)[never] == 4).all(), (store, algo)
        for r in recs[never]:
            assert r.tobytes()[4:] == bytes(60)
        for r in recs[~never]:
            assert int(r["status"]) == pick_ref.VOXEL and np.isnan(r["point"]).all()
        seen[(store, algo)] = int(np.count_nonzero(never))
        sc.close()
    assert seen == {(0, 1): 16, (0, 0): 0, (1, 1): 16, (1, 0): 0}
