"""GPU tests of vr_scene_lookup / vr_scene_paint (include/vr.h, csrc/vr_access.hip).  A lookup
is set membership in the scene's voxel set for ANY int32 coordinates (tests/access_cases.py is
the model and makes the queries).  After a paint the scene's digest equals that of a
from-scratch build of the recoloured set and that of vr_scene_edit given the stored part of the
batch, failed paints change nothing, frames equal the oracle's, and -- unlike an edit -- the
next render still runs under the view's learned orders."""
from __future__ import annotations

import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import oracle
from tests.access_cases import INT32_MAX, INT32_MIN, VOXEL_ABSENT, absent_in_box, frame_of, lookup_model, paint_model, queries
from tests.edit_cases import VOXEL_REMOVE, apply_edits, split_case
from tests.fuzz_cases import make_case, make_wide_case
from tests.helpers import diff_report, gpu_render, oracle_camera_from, oracle_lighting_from
from tests.test_gpu_edit import same_scene
from tests.test_gpu_parity import check_frame

pytestmark = pytest.mark.gpu

vr = pytest.importorskip("voxelraymarcher_amd")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "voxelraymarcher_amd", "bin", "VoxelRaymarcher")

VCS, HASH = vr.StorageType.VOXEL_CLUSTER_STORE, vr.StorageType.HASH_TABLE
STORES = [VCS, HASH]
ALGOS = [vr.RayMarchAlgorithm.ORIGINAL, vr.RayMarchAlgorithm.LONGEST_AXIS]
CASES = [("case", s) for s in range(12)] + [("wide", s) for s in range(4)]
FRAME_CASES = [("case", 3), ("case", 7), ("wide", 1)]


@functools.lru_cache(maxsize=None)
def case(kind, seed):
    """The fuzz case, its voxel set (duplicates resolved), the generator's queries for it (a
    count that is no multiple of 64) and the model's answers, made once."""
    c = make_wide_case(seed) if kind == "wide" else make_case(seed)
    xyz, rgb = apply_edits(c.xyz[:0], c.rgb[:0], c.xyz, c.rgb)
    q = queries(xyz, np.random.default_rng(1000 + seed))
    if len(q) % 64 == 0:
        q = q[:-1]
    return c, xyz, rgb, q, lookup_model(xyz, rgb, q)


def lookup_both_ways(scene, q):
    """scene.lookup(q) with host arrays and with a device tensor: the same words."""
    host = scene.lookup(q)
    assert isinstance(host, np.ndarray) and host.dtype == np.uint32 and host.shape == (len(q),)
    dev = scene.lookup(torch.from_numpy(np.ascontiguousarray(q, dtype=np.int32)).cuda())
    assert dev.is_cuda and dev.dtype == torch.int32 and tuple(dev.shape) == (len(q),)
    assert np.array_equal(dev.cpu().numpy().view(np.uint32), host), "device tensors and host arrays disagree"
    return host


def wrong(got, want, q):
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return "identical"
    i = int(bad[0])
    return f"{bad.size} of {len(q)} lookups differ, first at {q[i].tolist()}: got {got[i]:#x}, want {want[i]:#x}"


# ------------------------------------------------------------------------------------ lookup
@pytest.mark.parametrize("store", STORES, ids=lambda s: s.name)
@pytest.mark.parametrize("kind,seed", CASES)
def test_lookup_matches_the_model(kind, seed, store):
    _, xyz, rgb, q, want = case(kind, seed)
    with vr.create_scene(xyz, rgb, store) as scene:
        got = lookup_both_ways(scene, q)
        assert np.array_equal(got, want), wrong(got, want, q)
        for n in (1, 63, 65):
            got = lookup_both_ways(scene, q[:n])
            assert np.array_equal(got, want[:n]), f"n = {n}: " + wrong(got, want[:n], q[:n])


def directed_vcs_voxels():
    """Two occupied regions, (0,0,0) and (2,0,0), with the null region (1,0,0) between them.  The
    cluster at (8,16,24) holds in-cluster indices 0, 31, 32, 63 and 511 (bits 0 and 31, words 0, 1
    and 15); clusters with distinct x>>3, y>>3, z>>3 and their x/z mirror images hold other
    colours; region (2,0,0) repeats two of them, so that a region index >= 1 is addressed."""
    cluster = [(0, 0, 0), (0, 3, 7), (0, 4, 0), (0, 7, 7), (7, 7, 7)]          # q = 0, 31, 32, 63, 511
    xyz = [(8 + a, 16 + b, 24 + c) for a, b, c in cluster]
    xyz += [(24, 16, 8), (25, 17, 9), (40, 16, 8), (8, 32, 24), (56, 8, 0), (0, 8, 56)]
    xyz += [(128 + 8, 16, 24), (128 + 24, 16, 8), (128 + 63, 63, 63)]
    return np.array(xyz, dtype=np.int32), (0x010203 + 0x010101 * np.arange(len(xyz))).astype(np.uint32)


@pytest.mark.parametrize("store", STORES, ids=lambda s: s.name)
def test_lookup_directed_cluster_scene(store):
    xyz, rgb = directed_vcs_voxels()
    absent = [(8, 16, 25), (8, 19, 30), (8, 20, 25), (15, 23, 30), (9, 16, 24),    # q = 1, 30, 33, 510, 64 of the cluster
              (24, 16, 24), (8, 16, 40), (8, 16, 8), (24, 32, 24),                  # absent clusters of region (0,0,0)
              (64 + 8, 16, 24), (64 + 24, 16, 8), (64, 0, 0), (127, 63, 63),        # the null region between
              (128 + 24, 16, 24), (128 + 8, 16, 25), (128, 0, 0),                   # region (2,0,0)
              (8, 64, 24), (8, 16, 64 + 24), (191, 191, 191),                       # other null regions of the frame
              (192, 0, 0), (-1, 0, 0), (8, -48, 24), (8, 16, 192), (0, 0, -1)]      # outside the frame
    q = np.concatenate([xyz, np.array(absent, dtype=np.int32)])
    with vr.create_scene(xyz, rgb, store) as scene:
        assert scene.info()["region_count"] == 2 and scene.info()["diameter"] == 3
        got = lookup_both_ways(scene, q)
    assert np.array_equal(got[: len(xyz)], rgb), wrong(got[: len(xyz)], rgb, xyz)
    assert np.all(got[len(xyz):] == VOXEL_ABSENT), wrong(got, lookup_model(xyz, rgb, q), q)
    assert got[0] != got[5]          # (8,16,24) and its x/z mirror (24,16,8)


@pytest.mark.parametrize("store", STORES, ids=lambda s: s.name)
def test_lookup_directed_table_scene(store):
    """A region with one voxel (a cuckoo table of one slot per half) beside a region of about
    3000 random voxels, whose keys lie in both tables: every stored key is found, 3000 absent
    keys of the same regions are not."""
    rng = np.random.default_rng(7)
    big = np.unique(rng.integers(0, 64, size=(3000, 3)), axis=0) + np.array([64, 0, 0])
    xyz = np.concatenate([np.array([[5, 6, 7]]), big]).astype(np.int32)
    rgb = rng.integers(0, 1 << 24, size=len(xyz), dtype=np.uint32)
    gone = np.concatenate([absent_in_box(big, 3000, rng), rng.integers(0, 64, size=(200, 3)).astype(np.int32)])
    gone = gone[~np.all(gone == np.array([5, 6, 7]), axis=1)]
    with vr.create_scene(xyz, rgb, store) as scene:
        got = lookup_both_ways(scene, xyz)
        assert np.array_equal(got, rgb), wrong(got, rgb, xyz)
        got = lookup_both_ways(scene, gone)
        assert np.all(got == VOXEL_ABSENT), wrong(got, np.full(len(gone), VOXEL_ABSENT, dtype=np.uint32), gone)


@pytest.mark.parametrize("store", STORES, ids=lambda s: s.name)
@pytest.mark.parametrize("kind,seed", FRAME_CASES)
def test_lookup_round_trips_through_edit(kind, seed, store):
    c, xyz, rgb, q, _ = case(kind, seed)
    with vr.create_scene(xyz, rgb, store) as scene:
        # edit(q, lookup(q)) changes nothing (VOXEL_ABSENT is VOXEL_REMOVE); an edit takes
        # coordinates inside the frame only
        info = scene.info()
        lo, hi = info["min_coord"] * 64, (info["min_coord"] + info["diameter"]) * 64
        assert (lo, hi) == frame_of(xyz)
        inside = q[np.all((q >= lo) & (q < hi), axis=1)]
        before = scene.digest()
        scene.edit(inside, scene.lookup(inside))
        assert scene.digest() == before
    # after a real edit with insertions and removals, lookups are the edited set's
    ixyz, irgb, exyz, ergb, _ = split_case(c.xyz, c.rgb, np.random.default_rng(seed))
    nxyz, nrgb = apply_edits(ixyz, irgb, exyz, ergb)
    nq = np.concatenate([queries(nxyz, np.random.default_rng(seed)), exyz])
    with vr.create_scene(ixyz, irgb, store) as scene:
        scene.edit(exyz, ergb)
        got, want = lookup_both_ways(scene, nq), lookup_model(nxyz, nrgb, nq)
        assert np.array_equal(got, want), wrong(got, want, nq)


@pytest.mark.parametrize("store", STORES, ids=lambda s: s.name)
def test_the_empty_scene(store):
    empty = np.zeros((0, 3), dtype=np.int32), np.zeros(0, dtype=np.uint32)
    q = queries(empty[0], np.random.default_rng(0))
    with vr.create_scene(*empty, store) as scene:
        assert scene.info()["voxel_count"] == 0
        before = scene.digest()
        assert np.all(lookup_both_ways(scene, q) == VOXEL_ABSENT)
        assert scene.paint(q, np.full(len(q), 0x123456, dtype=np.uint32)) == len(q)
        assert scene.digest() == before
        assert scene.lookup(q[:0]).shape == (0,) and scene.paint(q[:0], np.zeros(0, dtype=np.uint32)) == 0


# ------------------------------------------------------------------------------------- paint
@functools.lru_cache(maxsize=None)
def paint_batch(kind, seed):
    """(exyz, ergb) for the case's voxel set: recolours of about a quarter of the stored voxels
    (at least 80 edits), 20 absent coordinates -- 10 inside the bounding box, 10 outside the
    frame -- shuffled, and three coordinates painted three times each: once each at indices
    0-2, at 70-72 (another wave) and at the last three, with colours that ascend, descend and
    do neither over the three edits."""
    _, xyz, rgb, _, _ = case(kind, seed)
    rng = np.random.default_rng(2000 + seed)
    assert len(xyz) >= 8
    order = rng.permutation(len(xyz))
    thrice, rest = order[:3], order[3:]
    stored = xyz[rest[: max(len(xyz) // 4, min(len(rest), 80))]]
    lo, hi = frame_of(xyz)
    outside = [(lo - 1, lo, lo), (hi, lo, lo), (lo, lo - 64, lo), (lo, hi + 63, hi - 1), (lo, lo, lo - 1), (hi - 1, lo, hi),
               (INT32_MIN, INT32_MIN, INT32_MIN), (INT32_MAX, INT32_MAX, INT32_MAX), (INT32_MAX, lo, lo), (lo, INT32_MIN, lo)]
    body = np.concatenate([stored, absent_in_box(xyz, 10, rng), np.array(outside, dtype=np.int64).astype(np.int32)])
    body = body[rng.permutation(len(body))]
    assert len(body) >= 76
    colours = rng.integers(0, 1 << 24, size=len(body), dtype=np.uint32)
    three = xyz[thrice]
    lo_c, mid_c, hi_c = 0x000010, 0x400000, 0xFFFFF0
    by_round = [(lo_c, hi_c, hi_c - 1), (mid_c, mid_c, lo_c + 1), (hi_c, lo_c, mid_c + 1)]   # A ascends, B descends, C: hi, lo, mid
    exyz = np.concatenate([three, body[:67], three, body[67:], three])
    ergb = np.concatenate([np.array(by_round[0], dtype=np.uint32), colours[:67], np.array(by_round[1], dtype=np.uint32),
                           colours[67:], np.array(by_round[2], dtype=np.uint32)])
    assert np.array_equal(exyz[70:73], three) and np.array_equal(exyz[-3:], three) and np.array_equal(exyz[:3], three)
    return np.ascontiguousarray(exyz), ergb


def stored_part(xyz, exyz, ergb):
    have = set(map(tuple, xyz.tolist()))
    keep = np.array([c in have for c in map(tuple, exyz.tolist())])
    return exyz[keep], ergb[keep]


def check_paint(scene, kind, seed, store, device_tensors=False):
    _, xyz, rgb, _, _ = case(kind, seed)
    exyz, ergb = paint_batch(kind, seed)
    pxyz, prgb, n_absent = paint_model(xyz, rgb, exyz, ergb)
    assert n_absent == 20
    info = scene.info()
    if device_tensors:
        got_absent = scene.paint(torch.from_numpy(exyz).cuda(), torch.from_numpy(ergb.astype(np.int64)).cuda())
    else:
        got_absent = scene.paint(exyz, ergb)
    assert got_absent == n_absent
    assert scene.info() == info
    with vr.create_scene(pxyz, prgb, store) as want:
        same_scene(scene, want, "paint vs a from-scratch build of the recoloured set")
    with vr.create_scene(xyz, rgb, store) as twin:
        twin.edit(*stored_part(xyz, exyz, ergb))
        same_scene(scene, twin, "paint vs edit of the stored part of the batch")
    got = scene.lookup(exyz)
    want = lookup_model(pxyz, prgb, exyz)
    assert np.array_equal(got, want), wrong(got, want, exyz)


@pytest.mark.parametrize("store", STORES, ids=lambda s: s.name)
@pytest.mark.parametrize("kind,seed", CASES)
def test_paint_digest(kind, seed, store):
    _, xyz, rgb, _, _ = case(kind, seed)
    with vr.create_scene(xyz, rgb, store) as scene:
        check_paint(scene, kind, seed, store)


@pytest.mark.parametrize("store", STORES, ids=lambda s: s.name)
def test_paint_device_tensors_and_host_built_scene(store):
    _, xyz, rgb, _, _ = case("case", 3)
    with vr.create_scene(xyz, rgb, store) as scene:
        check_paint(scene, "case", 3, store, device_tensors=True)
    with vr.create_scene(xyz, rgb, store, build=vr.Build.HOST) as scene:
        check_paint(scene, "case", 3, store)
    with vr.create_scene(xyz, rgb, store, build=vr.Build.HOST) as scene:
        check_paint(scene, "case", 3, store, device_tensors=True)


@pytest.mark.parametrize("store", STORES, ids=lambda s: s.name)
def test_failed_paints_change_nothing(store):
    _, xyz, rgb, _, _ = case("case", 5)
    exyz, ergb = paint_batch("case", 5)
    with vr.create_scene(xyz, rgb, store) as scene:
        before, info = scene.digest(), scene.info()
        for bad in (1 << 24, VOXEL_REMOVE):
            bad_rgb = ergb.copy()
            bad_rgb[5] = bad
            bad_rgb[-1] = bad                   # (the FIRST bad index is named)
            for dev in (False, True):
                args = (torch.from_numpy(exyz).cuda(), torch.from_numpy(bad_rgb.astype(np.int64)).cuda()) if dev \
                    else (exyz, bad_rgb)
                with pytest.raises(vr.VrError) as e:
                    scene.paint(*args)
                assert e.value.code == -1 and "index 5 " in str(e.value) and "vr_scene_paint" in str(e.value)
                assert str(bad) in str(e.value)
                assert scene.digest() == before and scene.info() == info
        # a capturing stream
        dxyz, drgb = torch.from_numpy(exyz).cuda(), torch.from_numpy(ergb.astype(np.int64)).cuda().to(torch.int32)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        err = None
        with torch.cuda.graph(g, stream=s):
            try:
                scene.paint(dxyz, drgb, stream=s)
            except vr.VrError as ex:
                err = ex
        assert err is not None and err.code == -1 and "captur" in str(err)
        torch.cuda.synchronize()
        assert scene.digest() == before and scene.info() == info
        # the scene still takes the batch afterwards
        assert scene.paint(exyz, ergb) == 20
        assert scene.digest() != before


def view_of(c, W, H):
    cam = vr.Camera(c.eye, c.look_at, c.up, c.fov, float(np.float32(W) / np.float32(H)))
    lit = vr.setup_constant_values(use_shadows=c.shadows, use_point_light=c.point, light_position=c.light_pos,
                                   light_direction=c.light_dir, light_color=c.light_color)
    return cam, lit, vr.VoxelSceneInfo(c.translation, c.scale)


@pytest.mark.parametrize("store", STORES, ids=lambda s: s.name)
@pytest.mark.parametrize("kind,seed", FRAME_CASES)
def test_frames_of_the_painted_scene(kind, seed, store):
    c, xyz, rgb, _, _ = case(kind, seed)
    exyz, ergb = paint_batch(kind, seed)
    pxyz, prgb, _ = paint_model(xyz, rgb, exyz, ergb)
    W, H = min(c.W, 48), min(c.H, 40)
    cam, lit, info = view_of(c, W, H)
    ref = oracle.Scene(pxyz, prgb, int(store))
    gpu = vr.create_scene(xyz, rgb, store)
    gpu.paint(exyz, ergb)
    for algo in ALGOS:
        want, wbytes = ref.render(int(algo), oracle_camera_from(cam), oracle_lighting_from(lit), W, H, c.scale,
                                  c.translation)
        got, gbytes = gpu_render(gpu, algo, cam, lit, info, W, H, count=True)
        assert np.array_equal(got, want), f"{algo.name}: " + diff_report(got, want, W)
        assert gbytes == wbytes, f"{algo.name}: algorithmic bytes: gpu {gbytes} != oracle {wbytes}"
        # and under the learned lane and work orders of the painted scene's view (check_frame)
        check_frame(pxyz, prgb, store, algo, W, H, c.scale, cam=cam, lit=lit, translation=c.translation,
                    gpu_scene=gpu, want=(want, wbytes))
    gpu.close()
    ref.close()


def learned_view(scene, algo, cam, lit, info, W, H, device):
    """Render the view until it is under its learned orders (slots + 2 launches), check that the
    next launch has a lane order bound, and return that frame."""
    vr.forget_orders(device)
    for _ in range(vr.debug_order_uses(device)["slots"] + 2):
        gpu_render(scene, algo, cam, lit, info, W, H)
    bound = vr.debug_order_uses(device)["lane_order_uses"]
    frame, _ = gpu_render(scene, algo, cam, lit, info, W, H)
    assert vr.debug_order_uses(device)["lane_order_uses"] == bound + 1, "the view is not under its learned orders"
    return frame


@pytest.mark.parametrize("store,algo", [(VCS, ALGOS[0]), (HASH, ALGOS[1])], ids=lambda p: p.name)
def test_learned_orders_survive_a_paint_but_not_an_edit(store, algo):
    c, xyz, rgb, _, _ = case("case", 3)
    W, H = min(c.W, 48), min(c.H, 40)
    cam, lit, info = view_of(c, W, H)
    ys, xs = np.mgrid[0:H, 0:W]
    with vr.create_scene(xyz, rgb, store) as scene, vr.create_scene(xyz, rgb, store) as twin:
        device = scene.info()["device"]
        hits = scene.pick(algo, cam, info, W, H, xs.reshape(-1).astype(np.uint32), ys.reshape(-1).astype(np.uint32))
        seen = hits[hits["status"] == int(vr.HitStatus.VOXEL)]
        assert len(seen), "the view shows no voxel"
        voxel = seen["voxel"][:1].astype(np.int32)
        colour = np.array([int(seen["color"][0]) ^ 0xFFFFFF], dtype=np.uint32)
        pxyz, prgb, n_absent = paint_model(xyz, rgb, voxel, colour)
        assert n_absent == 0
        ref = oracle.Scene(pxyz, prgb, int(store))
        want, _ = ref.render(int(algo), oracle_camera_from(cam), oracle_lighting_from(lit), W, H, c.scale, c.translation)
        ref.close()
        # paint: the very next launch is still under the view's lane order, and shows the new colour
        learned_view(scene, algo, cam, lit, info, W, H, device)
        assert scene.paint(voxel, colour) == 0
        bound = vr.debug_order_uses(device)["lane_order_uses"]
        got, _ = gpu_render(scene, algo, cam, lit, info, W, H)
        assert vr.debug_order_uses(device)["lane_order_uses"] == bound + 1, "the paint unbound the learned lane order"
        assert np.array_equal(got, want), diff_report(got, want, W)
        # the contrast: the same recolour through edit makes the next launch a first render
        learned_view(twin, algo, cam, lit, info, W, H, device)
        twin.edit(voxel, colour)
        bound = vr.debug_order_uses(device)["lane_order_uses"]
        got, _ = gpu_render(twin, algo, cam, lit, info, W, H)
        assert vr.debug_order_uses(device)["lane_order_uses"] == bound, "an edit is expected to unbind the lane order"
        assert np.array_equal(got, want), diff_report(got, want, W)


# --------------------------------------------------------------------------------------- CLI
def cli(tmp_path, store, *extra):
    _, xyz, rgb, _, _ = case("case", 3)
    scene_path = str(tmp_path / "scene.vxb")
    vr.write_binary_scene(scene_path, xyz, rgb)
    args = [EXE, "1", store, "original", "--scene", scene_path, "--width", "64", "--height", "48", "--out",
            str(tmp_path / "output.png"), *extra]
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return [ln for ln in r.stdout.splitlines() if ln.startswith("lookup ")], r.stderr, r.stdout.splitlines()


@pytest.mark.parametrize("store", ["vcs", "hashtable"])
def test_cli_lookup(tmp_path, store):
    _, xyz, rgb, _, _ = case("case", 3)
    x, y, z = (int(v) for v in xyz[0])
    gone = absent_in_box(xyz, 1, np.random.default_rng(0))[0]
    got, _, lines = cli(tmp_path, store, "--lookup", f"{x},{y},{z}", "--lookup", f"{gone[0]},{gone[1]},{gone[2]}",
                        "--lookup", "-1,-64,-65000")
    assert got == [f"lookup {x} {y} {z} color 0x{int(rgb[0]):06X}", f"lookup {gone[0]} {gone[1]} {gone[2]} absent",
                   "lookup -1 -64 -65000 absent"]
    order = [ln.split()[0] for ln in lines if ln.startswith(("Execution Time", "lookup ", "Wrote "))]
    assert order == ["Execution", "lookup", "lookup", "lookup", "Wrote"]


def test_cli_refusals(tmp_path):
    """Both flags are refused where they cannot mean what they say, before anything is rendered."""
    base = [EXE, "1", "vcs", "original", "--synth", "64", "--width", "64", "--height", "64", "--out", str(tmp_path / "o.png")]
    for flag, value, gpus in (("--lookup", "1,2,3", "2"), ("--paint", "1,2,3,FF00FF", "2"), ("--paint", "1,2,3,FF00FF", "1")):
        r = subprocess.run(base + ["--gpus", gpus, flag, value], capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and flag in r.stderr, r.stdout + r.stderr
    for flag, value in (("--lookup", "1,2"), ("--lookup", "1,2,3,4"), ("--lookup", "1,2,2147483648"), ("--paint", "1,2,3"),
                        ("--paint", "1,2,3,-1"), ("--paint", "1,2,3,GG")):
        r = subprocess.run(base + [flag, value], capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and f"{flag} needs" in r.stderr, r.stdout + r.stderr
    # a colour above 24 bits reaches vr_scene_paint, which refuses the batch
    r = subprocess.run(base + ["--paint", "1,2,3,1000000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "vr_scene_paint" in r.stderr and "index 0 " in r.stderr, r.stdout + r.stderr
    assert not os.path.exists(tmp_path / "o.png")


@pytest.mark.parametrize("store", ["vcs", "hashtable"])
def test_cli_paint_then_lookup(tmp_path, store):
    _, xyz, rgb, _, _ = case("case", 3)
    x, y, z = (int(v) for v in xyz[1])
    got, err, _ = cli(tmp_path, store, "--paint", f"{x},{y},{z},12ab", "--paint", "-70,5,5,FFFFFF", "--paint",
                      f"{x},{y},{z},ABCDEF", "--lookup", f"{x},{y},{z}", "--lookup", "-70,5,5")
    assert got == [f"lookup {x} {y} {z} color 0xABCDEF", "lookup -70 5 5 absent"]
    assert "paint -70 5 5 absent" in err
    assert os.path.exists(tmp_path / "output.png")
