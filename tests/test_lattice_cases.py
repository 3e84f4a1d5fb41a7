"""CPU preconditions of the lattice cases (tests/lattice_cases.py): that the walks do start on
the lattice, that the numpy reference (tests/pick_ref.py, tests/trace_ref.py) still agrees with
the C oracle there -- where a numpy `floor` and C's could part -- and that the views and ray
families are not vacuous, before tests/test_gpu_lattice.py judges the kernels with them.

What the reference does at exact planes, as these tests find it:
  * the frame's upper face (128) is outside the frame: every walk from it is background after
    one iteration; the lower face (-64) is inside
  * the original walk never hits along a direction with a zero component: its first step divides
    by that component without a guard, floor(o) - EPSILON - o is negative wherever o is (on the
    lattice or not), so the step is -inf and the ray leaves the region.  The longest-axis walk
    does hit along such directions -- one reason why the two algorithms disagree about which rays
    hit on 7 to 8 % of the lattice rays
  * the longest-axis walk's hit point has an exactly integer component in over a quarter of its
    components; the original walk's has none

Per (store, algorithm) the tests print the reference's MISS / VOXEL / NEVER counts and longest
walk of every family and view (pytest -s)."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import oracle
from tests import edge_cases as ec
from tests import lattice_cases as lc
from tests import pick_ref, trace_ref
from tests.test_edge_cases import oracle_camera, oracle_lighting
from tests.test_pick_ref import check_against_oracle

F = np.float32
PAIRS = [(s, a) for s in (oracle.STORE_VCS, oracle.STORE_HASHTABLE) for a in (oracle.ALGO_ORIGINAL, oracle.ALGO_LONGESTAXIS)]
PAIR_ID = lambda p: f"{'vcs' if p[0] == 0 else 'hash'}-{'original' if p[1] == 1 else 'longest'}"   # noqa: E731
NAMES = list(lc.VIEWS)
LONG_WALK = 65536
MIN_LIT, MIN_COLOURS = 200, 100
MAX_REFERENCE_ITERS = 10 ** 6
AXES = {d for d in lc.AXIS_DIRS if sum(c != 0 for c in d) == 1}


def view_lighting(v):
    return lc.set_point_light(oracle_lighting(v), v)


@functools.lru_cache(maxsize=None)
def facts(name):
    """Per store x algorithm the oracle's frame, bytes and per-pixel statistics of a view."""
    v = lc.VIEWS[name]
    cam, lit = oracle_camera(v), view_lighting(v)
    out = {}
    for store in (oracle.STORE_VCS, oracle.STORE_HASHTABLE):
        sc = oracle.Scene(v.xyz, v.rgb, store)
        for algo in (oracle.ALGO_ORIGINAL, oracle.ALGO_LONGESTAXIS):
            img, nbytes = sc.render(algo, cam, lit, v.W, v.H, v.scale, v.translation)
            st = sc.pixel_stats(algo, cam, lit, v.W, v.H, v.scale, v.translation)
            out[(store, algo)] = (img.reshape(v.H, v.W), nbytes, st)
        sc.close()
    return out


def counts(status):
    return tuple(int(np.count_nonzero(status == s)) for s in (trace_ref.MISS, trace_ref.VOXEL, trace_ref.NEVER))


# ---------------------------------------------------------------- the origins are on the lattice

def test_scene_and_view_list():
    xyz, _ = lc.scene_voxels()
    sc = oracle.Scene(*lc.scene_voxels(), 0)
    assert (sc.min_coord * 64, (sc.min_coord + sc.diameter) * 64) == (lc.FRAME_LO, lc.FRAME_HI)
    sc.close()
    assert xyz.min() == lc.LO and xyz.max() == lc.HI - 1
    planes = set(lc.PLANES)
    assert {0.0, 64.0, -64.0, float(lc.LO), float(lc.HI), float(lc.FRAME_LO), float(lc.FRAME_HI)} <= planes
    assert any(p % 8 == 0 and p % 64 != 0 for p in planes) and any(p % 8 != 0 for p in planes)
    assert any(p < lc.FRAME_LO for p in planes) and any(p > lc.FRAME_HI for p in planes)
    assert all(float(p).is_integer() for p in planes)
    vs = lc.VIEWS.values()
    assert all((v.W, v.H) == (64, 32) and v.raw is not None for v in vs)
    assert {v.axis for v in vs} == {0, 1, 2}
    zs = {v.plane for v in vs if v.axis == 2}
    assert {40.0, float(lc.FRAME_LO), float(lc.FRAME_HI)} <= zs and {0.0, 64.0, -64.0} & zs
    assert any(p % 8 == 0 and p % 64 != 0 for p in zs)
    assert any(v.step == 0.5 for v in vs) and any(v.scale == 2 and v.translation == lc.TRANSLATION for v in vs)
    shadowed = [v for v in vs if v.shadows and v.name != lc.UPPER_FACE]
    assert len(shadowed) >= 2 and any(v.point_light is not None for v in shadowed)
    lights = [ec.light(v) for v in shadowed]
    assert any((L == 0).any() for L in lights) and not any(L[0] == L[1] == L[2] for L in lights)
    assert set(lc.TIED) == set(lc.VIEWS) - {lc.LONG_CRAWL}


def test_frames_hold_whole_lane_blocks():
    import voxelraymarcher_amd as vr
    from tests.helpers import full_lane_blocks
    block = vr.debug_order_uses(0)["lane_block"]
    assert full_lane_blocks(lc.W, lc.H, block) == (lc.W // block[0]) * (lc.H // block[1]) == 4


@pytest.mark.parametrize("name", NAMES)
def test_view_origins_are_lattice_points(name):
    """Every pixel's origin, as trace_ref.camera_ray makes it and as the walk reads it
    ((origin - translation) * scale in float32), has its plane coordinate exactly on the plane and
    the other two exactly first + x * step and first + (H - y) * step: integers, or k + 0.5 at every
    other pixel of the half-step view."""
    v = lc.VIEWS[name]
    fields = pick_ref.cam_fields(oracle_camera(v))
    px, py = lc.frame_pixels()
    rays = np.array([trace_ref.camera_ray(fields, v.W, v.H, int(x), int(y)) for x, y in zip(px, py)])
    so = lc.scene_origins(rays, v.scale, v.translation)
    a, b = [i for i in range(3) if i != v.axis]
    assert (so[:, v.axis] == F(v.plane)).all() and float(v.plane).is_integer()
    assert np.array_equal(so[:, a], (v.first[0] + px * v.step).astype(F))
    assert np.array_equal(so[:, b], (v.first[1] + (v.H - py.astype(np.int64)) * v.step).astype(F))
    frac = so - np.floor(so)
    if v.step == 1.0:
        assert (frac == 0).all()
    else:
        assert v.step == 0.5 and set(np.unique(frac).tolist()) == {0.0, 0.5}
        assert (frac[:, a] == np.where(px % 2 == 1, 0.5, 0.0)).all()
    # the directions of the integer eyes are integer vectors before they are normalised
    if all(float(c).is_integer() for c in np.asarray(v.raw[0], F) * F(v.scale)) and v.scale == 1 and v.step == 1.0:
        assert (rays["direction"] == np.round(rays["direction"])).all()


def test_trace_origins_are_lattice_points():
    o, on, d = lc.lattice_points()
    assert len(o) == lc.N_RAYS >= 300
    assert np.isin(o[on], np.array(lc.PLANES, F)).all() and set(o[on].tolist()) == set(lc.PLANES)
    assert (o[~on] != np.round(o[~on])).all()
    assert sorted(set(on.sum(axis=1).tolist())) == [1, 2, 3]
    dirs = set(map(tuple, d.tolist()))
    assert {tuple(F(c) for c in x) for x in lc.AXIS_DIRS} <= dirs and len(lc.AXIS_DIRS) == 26
    obl = np.array(lc.OBLIQUE, F)
    assert (obl != 0).all() and set(ec.sign_pattern(obl).tolist()) == set(range(8))
    # every direction meets origins with one, two and three plane coordinates
    for x in dirs:
        assert set(on[(d == np.array(x, F)).all(axis=1)].sum(axis=1).tolist()) == {1, 2, 3}
    # one ulp to either side of one plane coordinate, nothing else moved
    no, moved, nd = lc.near_lattice_points()
    assert len(no) == 2 * len(o) and np.array_equal(nd, np.repeat(d, 2, axis=0))
    base = np.repeat(o, 2, axis=0)
    k = np.arange(len(no))
    assert on[k // 2, moved].all()
    assert ((no != base).sum(axis=1) == 1).all() and (no[k, moved] != base[k, moved]).all()
    m, b = no[k, moved], base[k, moved]
    assert (m[0::2] < b[0::2]).all() and (m[1::2] > b[1::2]).all()
    assert np.array_equal(np.nextafter(m, b), b)                           # exactly one ulp away
    assert np.count_nonzero(np.abs(m) < np.finfo(F).tiny) >= 2             # beside 0: the smallest subnormals


def test_scaled_forms_land_where_they_claim():
    """Scale 2 with TRANSLATION gives every plane coordinate back exactly; scale 3 gives some back
    and lands the others on a float32 within a few ulps of the plane: near-lattice origins of its
    own.  Of the near-lattice family scale 2 keeps some coordinates one ulp off and collapses
    others onto the plane (lc.maps_back tells which)."""
    o, on, _ = lc.lattice_points()
    rays = lc.lattice_rays()
    assert lc.maps_back(rays, 1, lc.ZERO).all()
    s2, tr2 = lc.FORMS["scale2"]
    back2 = lc.maps_back(rays, s2, tr2)
    assert back2[on].all()
    assert np.array_equal(lc.scene_origins(lc.family_rays("lattice", "scale2"), s2, tr2)[on], o[on])
    s3, tr3 = lc.FORMS["scale3"]
    so3 = lc.scene_origins(lc.family_rays("lattice", "scale3"), s3, tr3)
    exact = lc.maps_back(rays, s3, tr3)
    assert np.array_equal(exact, so3 == o)
    off = on & ~exact
    print(f"scale 3: {int((on & exact).sum())} plane coordinates exact, {int(off.sum())} beside the plane")
    assert (on & exact).sum() >= on.sum() // 10 and off.sum() >= on.sum() // 10
    assert (so3[off] != np.round(so3[off])).all()
    assert (np.abs(so3[off] - o[off]) <= 8 * np.spacing(F(max(abs(p) for p in lc.PLANES)))).all()
    near = lc.near_lattice_rays()
    no, moved, _ = lc.near_lattice_points()
    k = np.arange(len(no))
    kept = lc.maps_back(near, s2, tr2)[k, moved]
    so2 = lc.scene_origins(lc.family_rays("near", "scale2"), s2, tr2)[k, moved]
    print(f"scale 2, near-lattice: {int(kept.sum())} stay one ulp off, {int((~kept).sum())} land elsewhere")
    assert kept.sum() >= len(no) // 10 and (~kept).sum() >= len(no) // 10
    assert (so2[~kept] == np.repeat(o, 2, axis=0)[k, moved][~kept]).sum() >= len(no) // 10    # collapsed onto the plane


# ---------------------------------------------------------------- the numpy reference agrees with the oracle

def test_only_the_long_crawl_view_is_left_out():
    """The views whose picks are not tied to the oracle below are those that hold a walk of more
    than 65 536 iterations: at most two, and exactly the one lattice_cases names.  (The GPU is held
    to the oracle on them all the same: tests/test_gpu_lattice.py::test_lattice_views.)"""
    long = [n for n in NAMES if max(int(st[..., 6].max()) for _, _, st in facts(n).values()) > LONG_WALK]
    assert len(long) <= 2 and long == [lc.LONG_CRAWL]
    # (a primary walk: the view renders without shadows)
    assert max(int(st[..., 0, 6].max()) for _, _, st in facts(lc.LONG_CRAWL).values()) >= LONG_WALK


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_ID)
@pytest.mark.parametrize("name", lc.TIED)
def test_pick_reference_agrees_with_oracle(name, pair):
    """pick_ref.pick_pixels over every pixel, shaded by pick_ref.shade, is the oracle's pixel; a
    record is VOXEL exactly where the oracle counts a primary hit (test_pick_ref's tie)."""
    store, algo = pair
    v = lc.VIEWS[name]
    px, py = lc.frame_pixels()
    with np.errstate(all="ignore"):
        recs, iters = check_against_oracle(v.xyz, v.rgb, store, algo, oracle_camera(v), v.W, v.H, v.scale,
                                           v.translation, px.astype(np.int64), py.astype(np.int64),
                                           min_hits=0 if name == lc.UPPER_FACE else MIN_LIT)
    print(f"{name} {PAIR_ID(pair)}: MISS / VOXEL / NEVER {counts(recs['status'])}, longest walk {int(iters.max())}")
    st = facts(name)[pair][2]
    if not v.shadows:          # the same walks as the frame's: the oracle counts the same iterations
        assert np.array_equal(iters.reshape(v.H, v.W), st[..., 0, 6].astype(np.int64))


# ---------------------------------------------------------------- the views are not vacuous

@pytest.mark.parametrize("name", NAMES)
def test_views_are_lit_and_coloured(name):
    for pair, (img, nbytes, st) in facts(name).items():
        lit, colours = int(np.count_nonzero(img)), len(np.unique(img))
        hits = st[..., 0, 5] > 0
        print(f"{name} {PAIR_ID(pair)}: {lit} lit pixels, {colours} colours, {nbytes} bytes, MISS / VOXEL "
              f"{int((~hits).sum())} / {int(hits.sum())}, longest walk {int(st[..., 6].max())}")
        if name == lc.UPPER_FACE:
            assert not img.any() and nbytes == 4 * img.size          # background: the pixel writes alone
            assert (st[..., 0, 6] == 1).all() and not st[..., 1, :].any() and not hits.any()
        else:
            assert lit >= MIN_LIT and colours >= MIN_COLOURS, (name, pair, lit, colours)


def test_algorithms_differ_and_shadows_fall():
    differ = [n for n in NAMES if not np.array_equal(facts(n)[(0, oracle.ALGO_ORIGINAL)][0],
                                                      facts(n)[(0, oracle.ALGO_LONGESTAXIS)][0])]
    assert differ, "the original and the longest-axis frames are the same in every view"
    both = []
    for n in NAMES:
        if not lc.VIEWS[n].shadows or n == lc.UPPER_FACE:
            continue
        ok = True
        for pair, (img, _, st) in facts(n).items():
            walked = st[..., 1, 6] > 0                               # a shadow walk ran: a primary hit
            ok &= int((walked & (img == 0)).sum()) >= 32 and int((walked & (img != 0)).sum()) >= 32
        if ok:
            both.append(n)
    assert len(both) >= 2, both           # lit and shadowed hit pixels side by side, every pair


# ---------------------------------------------------------------- the ray families are not vacuous

@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_ID)
@pytest.mark.parametrize("form", list(lc.FORMS))
@pytest.mark.parametrize("family", list(lc.FAMILIES))
def test_ray_families(family, form, pair):
    store, algo = pair
    longest = algo == oracle.ALGO_LONGESTAXIS
    rays = lc.family_rays(family, form)
    with np.errstate(all="ignore"):
        recs, iters = lc.reference(family, form, store, longest)
    miss, voxel, never = counts(recs["status"])
    print(f"{family} {form} {PAIR_ID(pair)}: {len(rays)} rays, MISS / VOXEL / NEVER {miss} / {voxel} / {never}, "
          f"longest walk {int(iters.max())}, {int(iters.sum())} iterations in all")
    assert voxel >= len(rays) // 5 and miss >= len(rays) // 5
    assert int(iters.sum()) < MAX_REFERENCE_ITERS
    d = rays["direction"][recs["status"] == trace_ref.VOXEL]
    oblique = (d != 0).all(axis=1)
    assert set(ec.sign_pattern(d[oblique]).tolist()) == set(range(8))
    if longest:
        assert AXES <= set(map(tuple, d.tolist()))
    else:
        # no ray with a zero direction component hits (this module's docstring), so no axis
        # direction can occur among the original walk's hits: asserted as the reference has it
        assert oblique.all()
        assert np.count_nonzero((rays["direction"] == 0).any(axis=1)) >= len(rays) // 3


@pytest.mark.parametrize("store", (oracle.STORE_VCS, oracle.STORE_HASHTABLE), ids=("vcs", "hash"))
def test_algorithms_disagree_on_lattice_rays(store):
    with np.errstate(all="ignore"):
        a = lc.reference("lattice", "scale1", store, False)[0]["status"]
        b = lc.reference("lattice", "scale1", store, True)[0]["status"]
    share = float(np.mean(a != b))
    print(f"store {store}: the statuses differ on {100 * share:.1f} % of the lattice rays")
    assert share >= 0.05


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_ID)
@pytest.mark.parametrize("form", lc.BOUNCE_FORMS)
def test_bounce_rays(form, pair):
    store, algo = pair
    longest = algo == oracle.ALGO_LONGESTAXIS
    scale, tr = lc.FORMS[form]
    with np.errstate(all="ignore"):
        first, _ = lc.reference("lattice", form, store, longest)
        rays, src, recs, iters = lc.bounce_reference(form, store, longest)
    h = int(np.count_nonzero(first["status"] == trace_ref.VOXEL))
    assert len(rays) == 3 * h and h >= 100 and (first["status"][src] == trace_ref.VOXEL).all()
    # the origin is the hit point: on the hit voxel's face or within EPSILON's reach of it (the
    # original walk), or up to one step of the longest axis before it (the longest-axis walk
    # reports the position before the step that found the voxel)
    so = lc.scene_origins(rays, scale, tr)
    v = first["voxel"][src].astype(np.float64)
    assert (np.abs(so - (v + 0.5)).max(axis=1) <= (1.5 if longest else 0.5) + 1e-3).all()
    # reflected, the normal, reversed
    d, n = lc.family_rays("lattice", form)["direction"][src[:h]], first["normal"][src[:h]].astype(F)
    assert np.array_equal(rays["direction"][h:2 * h], n) and np.array_equal(rays["direction"][2 * h:], -d)
    refl = rays["direction"][:h]
    assert np.array_equal(np.where(n != 0, -d, d), refl)              # an axis normal flips one component
    miss, voxel, never = counts(recs["status"])
    on_lattice = float(np.mean(first["point"][src[:h]] == np.round(first["point"][src[:h]])))
    print(f"bounce {form} {PAIR_ID(pair)}: {len(rays)} rays, MISS / VOXEL / NEVER {miss} / {voxel} / {never}, longest "
          f"walk {int(iters.max())}, {int(iters.sum())} iterations; {100 * on_lattice:.0f} % of the hit points' "
          f"components are integers")
    assert voxel >= len(rays) // 5 and never == 0
    assert int(iters.sum()) < MAX_REFERENCE_ITERS
