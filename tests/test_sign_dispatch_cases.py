"""CPU preconditions of the sign-dispatch views (tests/sign_dispatch_cases.py): what makes them
tests of the per-ray sign dispatch and not an accident.  tests/test_gpu_sign_dispatch.py holds
the kernels to the oracle on these views; here numpy (the kernel's ray generation, restated in
float32 by tests/edge_cases.rays) and the oracle's per-pixel statistics say that

  * every view puts at least two sign patterns into one 8 x 8 tile (a wave then runs the
    walks of its patterns one after the other),
  * for every sign pattern of the view at least one ray walks two or more regions (the arm
    then runs more than one region round), and the patterns do not all cross equally many,
  * at least one ray meets the empty region (the null-region skip runs inside an arm),
  * the zero-column view has a direction component that is exactly 0."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import oracle
from tests import edge_cases as ec
from tests import sign_dispatch_cases as sd
from tests.test_edge_cases import oracle_camera, oracle_lighting

NAMES = list(sd.VIEWS)
REGION_READS, HITS = 0, 5            # columns of oracle.Scene.pixel_stats


@functools.lru_cache(maxsize=None)
def facts(name):
    c = sd.case(name, "noshadow")
    cam, lit = oracle_camera(c), oracle_lighting(c)
    ro, rd = ec.rays(ec.fields_of(cam), c.W, c.H)
    out = {"case": c, "ro": ro, "rd": rd, "pattern": ec.sign_pattern(rd), "stats": {}}
    for store in (oracle.STORE_VCS, oracle.STORE_HASHTABLE):
        sc = oracle.Scene(c.xyz, c.rgb, store)
        assert (sc.min_coord, sc.diameter) == (-1, 2)
        out["stats"][store] = sc.pixel_stats(oracle.ALGO_ORIGINAL, cam, lit, c.W, c.H, c.scale, c.translation)
        sc.close()
    return out


def test_scene_and_frame():
    xyz, _ = sd.scene()
    assert xyz.min() >= -64 and xyz.max() < 64
    reg = np.unique(xyz // 64, axis=0)
    assert len(reg) == 7 and not (reg == np.array(sd.EMPTY_REGION)).all(axis=1).any()
    # one whole 16 x 32 lane block at least, and blocks cut by the frame's edge
    assert sd.W // 16 >= 1 and sd.H // 32 >= 1 and sd.H % 32 != 0
    assert len(sd.LIGHTS) == 5


@pytest.mark.parametrize("name", NAMES)
def test_a_tile_holds_two_patterns(name):
    f = facts(name)
    per_tile = [len(np.unique(t)) for t in ec.tiles(f["pattern"])]
    print(f"{name}: patterns per tile {sorted(per_tile, reverse=True)[:6]}, in the frame {np.unique(f['pattern'])}")
    assert max(per_tile) >= 2
    if name != "zero-column":          # both image axes cross a sign change inside one tile
        assert max(per_tile) >= 3


@pytest.mark.parametrize("name", NAMES)
def test_each_pattern_walks_two_regions(name):
    f = facts(name)
    for store, st in f["stats"].items():
        reads = st[:, :, 0, REGION_READS]
        most = {}
        for p in np.unique(f["pattern"]):
            most[int(p)] = int(reads[f["pattern"] == p].max())
            assert most[int(p)] >= 2, (name, store, p, most)
        print(f"{name} store {store}: most regions read by a ray, per pattern: {most}")
        # (the rays of a tile do not all end in the same region round)
        mixed = [t for t, p in zip(ec.tiles(reads), ec.tiles(f["pattern"])) if len(np.unique(p)) >= 2]
        assert any(len(np.unique(t)) >= 2 for t in mixed), name


@pytest.mark.parametrize("name", NAMES)
def test_a_ray_meets_the_empty_region(name):
    """A ray that hits nothing walks region by region along its whole line through the scene:
    if that line passes through the inside of the empty region's box (slab test, with a margin
    far above any rounding), the walk made the null-region skip there."""
    f = facts(name)
    lo, hi = sd.empty_box()
    o = f["ro"].astype(np.float64)
    d = f["rd"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - o) / d, (hi - o) / d
    par = d == 0                                           # parallel to a slab: inside it or never
    inside = (o > lo) & (o < hi)
    near = np.where(par, np.where(inside, -np.inf, np.inf), np.minimum(t0, t1)).max(axis=-1)
    far = np.where(par, np.where(inside, np.inf, -np.inf), np.maximum(t0, t1)).min(axis=-1)
    through = (far - np.maximum(near, 0.0)) > 1.0          # more than one unit of length inside the box
    for store, st in f["stats"].items():
        miss = st[:, :, 0, HITS] == 0
        n = int((through & miss).sum())
        print(f"{name} store {store}: {n} rays cross the empty region and hit nothing")
        assert n >= 1
        assert (st[:, :, 0, REGION_READS][through & miss] >= 2).all()


def test_zero_column_is_exactly_zero():
    rd = facts("zero-column")["rd"]
    assert (rd[:, 23, 2] == 0).all() and (rd[:, 22, 2] < 0).all() and (rd[:, 24, 2] > 0).all()
    assert (rd[..., 1] > 0).any() and (rd[..., 1] < 0).any()
