"""CPU preconditions of the directed edge cases (tests/edge_cases.py): what makes each a test
of a guard and not an accident.  tests/test_gpu_edges.py holds the kernels to the oracle on
these cases; here the oracle itself (and the Python restatement beside it) says that the
cases leave vr::div_fast's domain where they mean to, by counts computed in numpy.float32 from
the camera fields as the kernel's ray generation computes them, that the out-of-domain rays
end in lit pixels (so a wrong quotient can change a visible word), that no walk leans on the
crawl pass or on a never-finishing walk, and that the frame is not all one colour."""
from __future__ import annotations

import functools
import os
import subprocess

import numpy as np
import pytest

import oracle
from tests import edge_cases as ec
from tests import pyref
from tests.test_oracle import _pyref_scene, _rays_agree
from tests.test_pick_ref import check_against_oracle

PAIRS = [(s, a) for s in (oracle.STORE_VCS, oracle.STORE_HASHTABLE) for a in (oracle.ALGO_ORIGINAL, oracle.ALGO_LONGESTAXIS)]
NAMES = list(ec.CASES)
MIN_LIT_OUT = 32          # out-of-domain rays that end in a lit pixel, per store x algorithm
MAX_ITERS = 20000         # per walk, primary or shadow
MIN_COLOURS = 8
PYREF_RAYS = 200          # per case, split over the four pairs; half from the out-of-domain set


def oracle_camera(c):
    if c.raw is not None:
        return ec.set_raw(oracle.OrCamera(), c)
    return oracle.camera(c.eye, c.look_at, c.up, c.fov, c.aspect)


def oracle_lighting(c):
    lit = oracle.lighting(use_shadows=c.shadows)
    L = ec.light(c)
    for i in range(3):
        lit.light_dir[i] = float(L[i])
        lit.light_color[i] = float(c.light_color[i])
    return lit


def pyref_lighting(c):
    plit = pyref.Lighting(c.shadows, False)
    if c.light_dir is not None:
        plit.L = pyref.V(*c.light_dir).unit()
    if c.raw_light is not None:
        plit.L = pyref.V(*c.raw_light)
    plit.LC = pyref.V(*c.light_color)
    return plit


@functools.lru_cache(maxsize=None)
def facts(name):
    """Everything the tests below read of a case, computed once: the rays, the out-of-domain
    sets, and per store x algorithm the oracle's frame and per-pixel statistics."""
    c = ec.CASES[name]
    cam = oracle_camera(c)
    lit = oracle_lighting(c)
    ro, rd = ec.rays(ec.fields_of(cam), c.W, c.H)
    L = ec.light(c)
    f = {"case": c, "cam": cam, "lit": lit, "rd": rd, "L": L, "dir_out": ec.divisor_out(rd).any(-1),
         "light_out": bool(ec.divisor_out(L).any()) and c.shadows, "frames": {}}
    for store, algo in [p for p in PAIRS if p[0] in c.stores]:
        sc = oracle.Scene(c.xyz, c.rgb, store)
        num, outside = ec.clip_numerators(ro, rd, c.scale, c.translation, sc.min_coord, sc.diameter)
        f["clip_out"] = ec.numerator_out(num).any(-1) & outside
        img, _ = sc.render(algo, cam, lit, c.W, c.H, c.scale, c.translation)
        st = sc.pixel_stats(algo, cam, lit, c.W, c.H, c.scale, c.translation)
        f["frames"][(store, algo)] = (img.reshape(c.H, c.W), st)
        sc.close()
    return f


def out_set(f):
    """The rays of the case's intended kind that leave the domain, [H, W] bool."""
    c = f["case"]
    if c.kind == "direction":
        return f["dir_out"]
    if c.kind == "clip":
        return f["clip_out"]
    if c.kind == "light":                 # every shadow ray divides by the light's components
        return np.full((c.H, c.W), f["light_out"])
    return np.zeros((c.H, c.W), dtype=bool)


def test_case_list():
    fams = {c.family for c in ec.CASES.values()}
    assert fams == {"E1", "E2", "E3", "E4", "E5", "E6", "E7", "E8"}
    for c in ec.CASES.values():
        assert (c.W, c.H) == (48, 32)
        assert np.isfinite(ec.light(c)).all() and np.isfinite(np.array(c.light_color, dtype=np.float32)).all()
        assert np.abs(c.xyz).max() < 2048
    assert len([c for c in ec.CASES.values() if c.family == "E4"]) == 6
    assert sorted(ec.PICK_CASES) == sorted(n for n, c in ec.CASES.items() if c.family in ("E1", "E3", "E5"))


def test_frames_hold_whole_lane_blocks():
    import voxelraymarcher_amd as vr
    from tests.helpers import full_lane_blocks
    block = vr.debug_order_uses(0)["lane_block"]
    for c in ec.CASES.values():
        assert full_lane_blocks(c.W, c.H, block) == (c.W // block[0]) * (c.H // block[1]) >= 1


@pytest.mark.parametrize("name", NAMES)
def test_out_of_domain_rays_are_lit(name):
    """The intended kind of out-of-domain ray is there, in the count the family promises, and at
    least 32 of them end in a lit pixel for every store x algorithm."""
    f = facts(name)
    c = f["case"]
    out = out_set(f)
    rd = f["rd"]
    n_out = int(out.sum())
    print(f"{name}: {n_out} of {out.size} rays out of the domain ({c.kind})")
    if c.family == "E1":
        assert 800 <= n_out <= 1000           # v * 0.8 < 0.5: 60 % of the rows
    if c.family == "E2":
        sub = (rd[..., 1] != 0) & (np.abs(rd[..., 1]) < ec.F32_MIN_NORMAL)
        assert n_out == out.size and int(sub.sum()) >= 300
    if c.family == "E3":
        two = ec.divisor_out(rd[..., 1]) & ec.divisor_out(rd[..., 2])
        # 2^-63: d.y leaves the domain in the rows with v < 1/2, d.z in the columns with u < 1/6
        assert int(two.sum()) >= (out.size if "124" in name else 100)
        if "124" in name:
            assert n_out == out.size and int(((np.abs(rd) < ec.F32_MIN_NORMAL) & (rd != 0)).any(-1).sum()) >= 300
    if c.family == "E4":
        L = f["L"]
        bad = ec.divisor_out(L)
        assert int(bad.sum()) == 1 and bad["xyz".index(name[-1])]
        assert (np.abs(L[bad]) < ec.F32_MIN_NORMAL).all() == ("130" in name)
    if c.family == "E8":
        L = f["L"]
        assert ec.divisor_out(L).all() and L[0] == L[1] == L[2]
    if c.family in ("E5", "E6"):
        assert n_out == out.size and not f["dir_out"].any()
    if c.kind == "signs":
        return
    for pair, (img, _) in f["frames"].items():
        lit_out = int((out & (img != 0)).sum())
        print(f"  {pair}: {lit_out} out-of-domain rays end in a lit pixel")
        assert lit_out >= MIN_LIT_OUT, (name, pair, lit_out)


def test_every_family_has_lit_out_of_domain_rays():
    for fam in ("E1", "E2", "E3", "E4", "E5", "E6", "E7", "E8"):
        best = {p: 0 for p in PAIRS}
        assert any(c.family == fam and len(c.stores) == 2 for c in ec.CASES.values())
        for n, c in ec.CASES.items():
            if c.family == fam:
                f = facts(n)
                for p, (img, _) in f["frames"].items():
                    best[p] = max(best[p], int((out_set(f) & (img != 0)).sum()))
        assert min(best.values()) >= MIN_LIT_OUT, (fam, best)


@pytest.mark.parametrize("name", [n for n, c in ec.CASES.items() if c.family in ("E1", "E7") and c.kind == "direction"])
def test_mixed_tiles(name):
    """At least 4 of the 24 8x8 tiles hold both in-domain and out-of-domain rays: the per-lane
    select behind the ballot has lanes on both arms."""
    t = ec.tiles(facts(name)["dir_out"])
    mixed = int((t.any(1) & ~t.all(1)).sum())
    assert mixed >= 4, mixed


def test_sign_patterns():
    """E7: the two shell views hold all 8 sign patterns between them (one camera cannot: see
    edge_cases.sign_cases), each with tiles that straddle one sign-change plane (2 patterns) and
    two (3 or 4); the mirrored E1 view has pattern-7 tiles with and without out-of-domain lanes,
    so both the P,P,P loop and the Sgn<2> loop run."""
    seen = set()
    for n in ("E7-signs-ppp", "E7-signs-nnn"):
        pat = ec.sign_pattern(facts(n)["rd"])
        seen |= set(pat.ravel().tolist())
        per_tile = np.array([len(set(t.tolist())) for t in ec.tiles(pat)])
        assert int((per_tile == 2).sum()) >= 4 and int((per_tile >= 3).sum()) >= 2, (n, per_tile.tolist())
        assert len(set(pat.ravel().tolist())) == 7
    assert seen == set(range(8))
    f = facts("E7-pattern7-tiny")
    p7, out = ec.tiles(ec.sign_pattern(f["rd"]) == 7), ec.tiles(f["dir_out"])
    assert int((p7 & out).any(1).sum()) >= 2             # pattern-7 lanes whose reciprocal is out of domain
    assert int((p7.all(1) & ~out.any(1)).sum()) >= 2     # whole pattern-7 tiles inside the domain


def test_shadow_rays_cover_every_sign_pattern():
    """The lights of the cases, between them, give shadow walks of all 8 sign patterns."""
    pats = {int(ec.sign_pattern(ec.light(c))) for c in ec.CASES.values() if c.shadows}
    assert pats == set(range(8))


@pytest.mark.parametrize("name", NAMES)
def test_walks_are_short_and_frames_coloured(name):
    f = facts(name)
    for pair, (img, st) in f["frames"].items():
        assert int(st[..., 6].max()) <= MAX_ITERS, (name, pair)
        colours = len(set(img.ravel().tolist()))
        if f["case"].family == "E3":
            # both tiny components put every ray on the one line y = z = +0 along -x: one voxel,
            # one colour, by geometry -- the frame must be lit all the same
            assert colours == 1 and img.all(), (name, pair)
        else:
            assert colours >= MIN_COLOURS, (name, pair, colours)


@pytest.mark.parametrize("name", NAMES)
def test_python_restatement_agrees(name):
    """tests/pyref.py and the oracle agree in colour and algorithmic bytes on sampled rays, half
    of them from the out-of-domain set (where there is one)."""
    f = facts(name)
    c = f["case"]
    rng = np.random.default_rng(sum(map(ord, name)))
    out = np.flatnonzero(out_set(f).ravel())
    per_pair = PYREF_RAYS // len(PAIRS)
    for store, algo in f["frames"]:
        half = per_pair // 2
        idx = rng.choice(out, half, replace=False) if len(out) >= half else np.zeros(0, dtype=np.int64)
        idx = np.concatenate([idx, rng.integers(0, c.W * c.H, per_pair - len(idx))])
        sc = oracle.Scene(c.xyz, c.rgb, store)
        ps = _pyref_scene(sc, c.xyz, c.rgb, store)
        with np.errstate(all="ignore"):
            _rays_agree(sc, ps, algo, f["cam"], f["lit"], pyref_lighting(c), c.W, c.H, c.scale,
                        (idx % c.W).astype(np.uint32), (idx // c.W).astype(np.uint32), translation=c.translation,
                        where=(name, store))
        sc.close()


@pytest.mark.parametrize("name", ec.PICK_CASES)
def test_pick_reference_agrees(name):
    """tests/pick_ref.py against the oracle on the cases test_gpu_edges.py picks (E1, E3, E5),
    as tests/test_pick_ref.py proves it on the other scenes, before it judges the kernel."""
    f = facts(name)
    c = f["case"]
    rng = np.random.default_rng(7)
    idx = rng.permutation(c.W * c.H)[:96]
    for store, algo in PAIRS:
        with np.errstate(all="ignore"):
            check_against_oracle(c.xyz, c.rgb, store, algo, f["cam"], c.W, c.H, c.scale, c.translation, idx % c.W,
                                 idx // c.W, min_hits=4)


def test_counting_build_is_apart_from_the_library():
    """libvr.so holds neither the counters nor their reader (vr_diag_fetch is no part of
    include/vr.h); libvr_cover.so, the same sources with -DVR_DIAG, holds both: the reader among
    its dynamic symbols (nm -D), the array in its symbol table (the host shadow of a __device__
    variable is a local symbol, which nm -D does not list; the device's copy sits in the code
    object)."""
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "voxelraymarcher_amd")

    def symbols(name, *flags):
        out = subprocess.run(["nm", *flags, os.path.join(pkg, name)], check=True, capture_output=True, text=True).stdout
        return {line.split()[-1] for line in out.splitlines() if line.strip()}
    lib, cover = symbols("libvr.so", "-D"), symbols("libvr_cover.so", "-D")
    assert "vr_diag_fetch" not in lib and "vr_diag_fetch" in cover
    assert "g_vr_diag" not in symbols("libvr.so") and "g_vr_diag" in symbols("libvr_cover.so")
    assert {s for s in lib if s.startswith("vr_")} <= cover      # the same ABI beside them


def test_no_jump_starts_in_a_negative_cell(monkeypatch):
    """The evidence beside the argument (vr_walk.h at the site) that the
    longest-axis walk's negative-cell cluster plane is never needed: over the alias fixture (whose
    walks do probe outside their region: the oracle counts them), a view made to leave a sparse
    block through its three low faces (edge_cases.low_face_case) and the tiny-direction cases
    that cross y = 0 and z = 0, the Python restatement never asks whether a cell with a negative
    coordinate exists -- and a jump starts only at a cell that was asked for."""
    import json

    from tests.helpers import GOLDEN
    from tests.test_oracle import _pyref_camera
    negative, asked = [], [0]
    plain = pyref.Walk.exists

    def exists(self, reg, x, y, z):
        asked[0] += 1
        if min(x, y, z) < 0:
            negative.append((x, y, z))
        return plain(self, reg, x, y, z)
    monkeypatch.setattr(pyref.Walk, "exists", exists)
    fx = json.load(open(os.path.join(GOLDEN, "alias_rays.json")))
    d = np.load(os.path.join(GOLDEN, fx["scene"]))
    sc, ps = oracle.Scene(d["xyz"], d["rgb"], 0), pyref.Scene(d["xyz"], d["rgb"], 0)
    outside = 0
    for c in fx["cameras"][:25]:
        cam = oracle.camera(c["eye"], c["at"], fx["up"], fx["fov"], fx["aspect"])
        outside += int(sc.pixel_stats(0, cam, oracle.lighting(), fx["width"], fx["height"], 1)[..., 7].sum())
        for i in range(fx["width"] * fx["height"]):
            pyref.render_pixel(ps, pyref.Lighting(), _pyref_camera(cam), fx["width"], fx["height"], i % fx["width"],
                               i // fx["width"], 1, True)
    assert outside >= 25                      # the fixture does probe outside the region ...
    low = ec.low_face_case()
    rng = np.random.default_rng(3)
    for c in (low, ec.CASES["E2-subnormal"], ec.CASES["E7-pattern7-tiny"]):
        cam = oracle_camera(c)
        sc, ps = oracle.Scene(c.xyz, c.rgb, 0), pyref.Scene(c.xyz, c.rgb, 0)
        st = sc.pixel_stats(0, cam, oracle_lighting(c), c.W, c.H, c.scale, c.translation)
        if c is low:
            assert int(st[..., 2].sum()) >= 1000 and int(st[..., 6].max()) <= MAX_ITERS   # cluster skips all the way
            assert (ec.rays(ec.fields_of(cam))[1] < 0).all()
        with np.errstate(all="ignore"):
            for i in rng.permutation(c.W * c.H)[:200]:
                pyref.render_pixel(ps, pyref_lighting(c), _pyref_camera(cam), c.W, c.H, int(i) % c.W, int(i) // c.W,
                                   c.scale, True, translation=c.translation)
    assert asked[0] > 10000
    assert not negative, negative[:5]         # ... but never at a negative cell
