"""GPU tests of vr_scene_edit / vr_scene_voxels (include/vr.h, csrc/vr_edit.hip): after an
edit the scene's digest equals that of a from-scratch build of the edited voxel set
(tests/edit_cases.py is the model), vr_scene_voxels returns that set, frames of the edited
scene equal the oracle's in pixels and algorithmic bytes, failed edits change nothing, and
the first render after an edit does not reuse what the renderer learned about the old
scene (the crawl-pass skip)."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import oracle
from tests.crawl_views import ASPECT, UP, VIEWS
from tests.crawl_views import H as CH
from tests.crawl_views import W as CW
from tests.crawl_views import points_scene
from tests.edit_cases import VOXEL_REMOVE, apply_edits, sort_voxels, split_case
from tests.fuzz_cases import make_case, make_wide_case
from tests.helpers import diff_report, gpu_render, oracle_camera_from, oracle_lighting_from
from tests.test_gpu_parity import check_frame

pytestmark = pytest.mark.gpu

vr = pytest.importorskip("voxelraymarcher_amd")

STORES = [vr.StorageType.VOXEL_CLUSTER_STORE, vr.StorageType.HASH_TABLE]
ALGOS = [vr.RayMarchAlgorithm.ORIGINAL, vr.RayMarchAlgorithm.LONGEST_AXIS]
CASES = [("case", s) for s in range(12)] + [("wide", s) for s in range(4)]
INFO_KEYS = ("diameter", "min_coord", "region_count", "voxel_count")


@functools.lru_cache(maxsize=None)
def case(kind, seed):
    """The fuzz case, its split (initial scene + batch) and the edited set, made once."""
    c = make_wide_case(seed) if kind == "wide" else make_case(seed)
    ixyz, irgb, exyz, ergb, _ = split_case(c.xyz, c.rgb, np.random.default_rng(seed))
    nxyz, nrgb = apply_edits(ixyz, irgb, exyz, ergb)
    return c, ixyz, irgb, exyz, ergb, nxyz, nrgb


def same_scene(got, want, what=""):
    gi, wi = got.info(), want.info()
    assert {k: gi[k] for k in INFO_KEYS} == {k: wi[k] for k in INFO_KEYS}, what
    assert gi["device_bytes"] == wi["device_bytes"], what
    assert got.digest() == want.digest(), f"{what}: digest differs from the from-scratch build"


def same_voxels(scene, xyz, rgb):
    gx, gc = sort_voxels(*scene.voxels())
    wx, wc = sort_voxels(xyz, rgb)
    assert np.array_equal(gx, wx) and np.array_equal(gc, wc)


@pytest.mark.parametrize("store", STORES, ids=lambda s: s.name)
@pytest.mark.parametrize("kind,seed", CASES)
def test_digest_and_round_trip(kind, seed, store):
    _, ixyz, irgb, exyz, ergb, nxyz, nrgb = case(kind, seed)
    want = vr.create_scene(nxyz, nrgb, store)
    one = vr.create_scene(ixyz, irgb, store)
    same_voxels(one, ixyz, irgb)
    one.edit(exyz, ergb)
    same_scene(one, want, "one edit")
    same_voxels(one, nxyz, nrgb)
    three = vr.create_scene(ixyz, irgb, store)
    cuts = [0, len(ergb) // 3, 2 * len(ergb) // 3, len(ergb)]
    for a, b in zip(cuts, cuts[1:]):
        three.edit(exyz[a:b], ergb[a:b])
    same_scene(three, want, "three consecutive edits")
    for s in (want, one, three):
        s.close()


@pytest.mark.parametrize("store", STORES, ids=lambda s: s.name)
def test_host_built_scene_and_device_tensor_edits(store):
    _, ixyz, irgb, exyz, ergb, nxyz, nrgb = case("case", 3)
    want = vr.create_scene(nxyz, nrgb, store)
    host = vr.create_scene(ixyz, irgb, store, build=vr.Build.HOST)
    host.edit(exyz, ergb)
    same_scene(host, want, "Build.HOST scene")
    dev = vr.create_scene(ixyz, irgb, store)
    dev.edit(torch.from_numpy(exyz).cuda(), torch.from_numpy(ergb.astype(np.int64)).cuda())
    same_scene(dev, want, "device tensors")
    dx, dc = dev.voxels(device=True)
    assert dx.is_cuda and dc.is_cuda and dx.shape == (len(nrgb), 3)
    gx, gc = sort_voxels(dx.cpu().numpy(), dc.cpu().numpy().view(np.uint32))
    wx, wc = sort_voxels(nxyz, nrgb)
    assert np.array_equal(gx, wx) and np.array_equal(gc, wc)
    hx, hc = dev.voxels()                       # the stated order is the same either way
    assert np.array_equal(hx, dx.cpu().numpy()) and np.array_equal(hc, dc.cpu().numpy().view(np.uint32))
    for s in (want, host, dev):
        s.close()


@pytest.mark.parametrize("store", STORES, ids=lambda s: s.name)
@pytest.mark.parametrize("kind,seed", CASES)
def test_frames_of_the_edited_scene(kind, seed, store):
    c, ixyz, irgb, exyz, ergb, nxyz, nrgb = case(kind, seed)
    W, H = min(c.W, 48), min(c.H, 40)
    cam = vr.Camera(c.eye, c.look_at, c.up, c.fov, float(np.float32(W) / np.float32(H)))
    lit = vr.setup_constant_values(use_shadows=c.shadows, use_point_light=c.point, light_position=c.light_pos,
                                   light_direction=c.light_dir, light_color=c.light_color)
    info = vr.VoxelSceneInfo(c.translation, c.scale)
    ref = oracle.Scene(nxyz, nrgb, int(store))
    gpu = vr.create_scene(ixyz, irgb, store)
    gpu.edit(exyz, ergb)
    for algo in ALGOS:
        want, wbytes = ref.render(int(algo), oracle_camera_from(cam), oracle_lighting_from(lit), W, H, c.scale,
                                  c.translation)
        got, gbytes = gpu_render(gpu, algo, cam, lit, info, W, H, count=True)
        assert np.array_equal(got, want), f"{algo.name}: " + diff_report(got, want, W)
        assert gbytes == wbytes, f"{algo.name}: algorithmic bytes: gpu {gbytes} != oracle {wbytes}"
        # and under the learned lane and work orders of the edited scene's view (check_frame)
        check_frame(nxyz, nrgb, store, algo, W, H, c.scale, cam=cam, lit=lit, translation=c.translation,
                    gpu_scene=gpu, want=(want, wbytes))
    gpu.close()
    ref.close()


def block(lo, size, seed):
    rng = np.random.default_rng(seed)
    xyz = (rng.integers(0, size, size=(300, 3)) + np.array(lo)).astype(np.int32)
    return xyz, rng.integers(0, 1 << 24, size=300, dtype=np.uint32)


@pytest.mark.parametrize("store", STORES, ids=lambda s: s.name)
def test_region_birth_and_death(store):
    """3 x 3 x 3 regions, the frame pinned by the corner voxels (0,0,0) and (191,191,191):
    one batch removes every voxel of region (1,0,0) and populates the null region (1,1,1)."""
    corners = np.array([[0, 0, 0], [191, 191, 191]], dtype=np.int32)
    dying = block((64, 0, 0), 64, 1)
    other = block((0, 128, 64), 64, 2)
    born = block((64, 64, 64), 64, 3)
    ixyz = np.concatenate([corners, dying[0], other[0]])
    irgb = np.concatenate([np.array([1, 2], dtype=np.uint32), dying[1], other[1]])
    exyz = np.concatenate([dying[0], born[0]])
    ergb = np.concatenate([np.full(len(dying[1]), VOXEL_REMOVE, dtype=np.uint32), born[1]])
    nxyz, nrgb = apply_edits(ixyz, irgb, exyz, ergb)
    scene = vr.create_scene(ixyz, irgb, store)
    assert scene.info()["region_count"] == 4 and scene.info()["diameter"] == 3
    scene.edit(exyz, ergb)
    want = vr.create_scene(nxyz, nrgb, store)
    same_scene(scene, want)
    assert scene.info()["region_count"] == 4
    same_voxels(scene, nxyz, nrgb)
    # and a batch that only empties a region: one region fewer
    scene.edit(born[0], np.full(len(born[1]), VOXEL_REMOVE, dtype=np.uint32))
    nxyz, nrgb = apply_edits(nxyz, nrgb, born[0], np.full(len(born[1]), VOXEL_REMOVE, dtype=np.uint32))
    want2 = vr.create_scene(nxyz, nrgb, store)
    same_scene(scene, want2)
    assert scene.info()["region_count"] == 3
    same_voxels(scene, nxyz, nrgb)
    for s in (scene, want, want2):
        s.close()


@pytest.mark.parametrize("store", STORES, ids=lambda s: s.name)
def test_edit_of_the_empty_scene(store):
    xyz, rgb = block((0, 0, 0), 64, 4)
    scene = vr.create_scene(np.zeros((0, 3), dtype=np.int32), np.zeros(0, dtype=np.uint32), store)
    assert scene.info()["voxel_count"] == 0 and scene.voxels()[0].shape == (0, 3)
    scene.edit(xyz, rgb)
    nxyz, nrgb = apply_edits(xyz[:0], rgb[:0], xyz, rgb)
    want = vr.create_scene(nxyz, nrgb, store)
    same_scene(scene, want)
    same_voxels(scene, nxyz, nrgb)
    # ... and back to empty
    scene.edit(xyz, np.full(len(rgb), VOXEL_REMOVE, dtype=np.uint32))
    empty = vr.create_scene(np.zeros((0, 3), dtype=np.int32), np.zeros(0, dtype=np.uint32), store)
    same_scene(scene, empty)
    for s in (scene, want, empty):
        s.close()


def test_cuckoo_rehash_is_drawn_as_in_the_build():
    """The scene of tests/test_oracle.py::test_rehashed_cuckoo_region_bytes_python_restatement:
    8 keys that share both default hash slots beside a dense block in the next region."""
    keys = [(0, 15, 63), (0, 36, 33), (0, 57, 6), (0, 60, 63), (3, 3, 45), (3, 12, 57), (3, 15, 48), (3, 45, 9)]
    g = np.stack(np.meshgrid(np.arange(64, 72), np.arange(0, 20), np.arange(20, 44), indexing="ij"), -1).reshape(-1, 3)
    xyz = np.concatenate([np.array(keys), g]).astype(np.int32)
    rgb = (np.arange(len(xyz), dtype=np.uint32) * 2654435761 % (1 << 24)).astype(np.uint32)
    store = vr.StorageType.HASH_TABLE
    ref = oracle.Scene(xyz, rgb, int(store))
    assert ref.cuckoo_table(0, 0)[1], "region 0 is expected to need a rehash"
    scene = vr.create_scene(xyz[8:], rgb[8:], store)
    scene.edit(xyz[:8], rgb[:8])
    want = vr.create_scene(xyz, rgb, store)
    same_scene(scene, want, "8 colliding keys inserted")
    W, H = 48, 40
    lit = vr.setup_constant_values(use_shadows=False)
    info = vr.VoxelSceneInfo((0.0, 0.0, 0.0), 1)
    for eye, at in (((-3.0, 40.0, 30.0), (4.0, 32.0, 30.0)), ((40.0, 70.0, 80.0), (2.0, 30.0, 30.0))):
        cam = vr.Camera(eye, at, (0.0, 1.0, 0.0), 70.0, W / H)
        for algo in ALGOS:
            wpix, wbytes = ref.render(int(algo), oracle_camera_from(cam), oracle_lighting_from(lit), W, H, 1)
            got, gbytes = gpu_render(scene, algo, cam, lit, info, W, H, count=True)
            assert np.array_equal(got, wpix), diff_report(got, wpix, W)
            assert gbytes == wbytes
    scene.edit(xyz[3:4], np.array([VOXEL_REMOVE], dtype=np.uint32))
    keep = np.arange(len(xyz)) != 3
    want7 = vr.create_scene(xyz[keep], rgb[keep], store)
    same_scene(scene, want7, "one of the 8 removed")
    for s in (scene, want, want7):
        s.close()
    ref.close()


@pytest.mark.parametrize("store", STORES, ids=lambda s: s.name)
def test_failed_edits_change_nothing(store):
    _, ixyz, irgb, exyz, ergb, _, _ = case("case", 5)
    scene = vr.create_scene(ixyz, irgb, store)
    before, info = scene.digest(), scene.info()
    n = len(ergb)
    # a colour of 2^24 in the last edit
    bad_rgb = ergb.copy()
    bad_rgb[-1] = 0x1000000
    with pytest.raises(vr.VrError) as e:
        scene.edit(exyz, bad_rgb)
    assert e.value.code == -1 and f"index {n - 1}" in str(e.value) and str(0x1000000) in str(e.value)
    assert scene.digest() == before and scene.info() == info
    # the last edit one region outside the frame
    bad_xyz = exyz.copy()
    bad_xyz[-1] = (info["min_coord"] + info["diameter"]) * 64, info["min_coord"] * 64, info["min_coord"] * 64
    with pytest.raises(vr.VrError) as e:
        scene.edit(bad_xyz, ergb)
    assert e.value.code == -1 and f"index {n - 1}" in str(e.value) and "frame" in str(e.value)
    assert scene.digest() == before and scene.info() == info
    bad_xyz[-1] = info["min_coord"] * 64 - 1, info["min_coord"] * 64, info["min_coord"] * 64
    with pytest.raises(vr.VrError) as e:
        scene.edit(bad_xyz, ergb)
    assert e.value.code == -1 and f"index {n - 1}" in str(e.value)
    assert scene.digest() == before
    # a capturing stream
    dxyz, drgb = torch.from_numpy(exyz).cuda(), torch.from_numpy(ergb.astype(np.int64)).cuda().to(torch.int32)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    err = None
    with torch.cuda.graph(g, stream=s):
        try:
            scene.edit(dxyz, drgb, stream=s)
        except vr.VrError as ex:
            err = ex
    assert err is not None and err.code == -1 and "captur" in str(err)
    torch.cuda.synchronize()
    assert scene.digest() == before and scene.info() == info
    # the scene still takes the batch afterwards
    scene.edit(exyz, ergb)
    assert scene.digest() != before
    scene.close()


def filler_voxels():
    """One voxel at local (3,3,3) of each of the 4096 clusters of [0,128)^3."""
    g = np.stack(np.meshgrid(*[np.arange(16)] * 3, indexing="ij"), -1).reshape(-1, 3) * 8 + 3
    return g.astype(np.int32), np.full(len(g), 0x808080, dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def points_frame(view_name, algo):
    view = next(v for v in VIEWS if v.name == view_name)
    xyz, rgb = points_scene()
    ref = oracle.Scene(xyz, rgb, oracle.STORE_VCS)
    cam = vr.Camera(view.world(view.eye), view.world(view.look_at), UP, view.fov, ASPECT)
    lit = vr.setup_constant_values()
    out = ref.render(int(algo), oracle_camera_from(cam), oracle_lighting_from(lit), CW, CH, view.scale, view.translation)
    ref.close()
    return out


@pytest.mark.parametrize("algo", ALGOS, ids=lambda a: a.name)
@pytest.mark.parametrize("view_name", ["z-plane", "x-plane-from-behind"])
def test_first_render_after_an_edit_runs_its_crawl_pass(view_name, algo):
    """With a voxel in every cluster no walk of the view skips a cluster, so nothing defers
    and, after 40 renders, every launch slot skips the view's crawl pass.  Removing the
    fillers in one edit leaves the plain `points` scene, whose view crawls for up to 10^6
    iterations: the very next render must run its crawl pass (vr_launch.cpp view_key hashes
    the scene's revision), or its deferred pixels are written as 0."""
    view = next(v for v in VIEWS if v.name == view_name)
    pxyz, prgb = points_scene()
    fxyz, frgb = filler_voxels()
    assert not set(map(tuple, pxyz.tolist())) & set(map(tuple, fxyz.tolist()))
    scene = vr.create_scene(np.concatenate([pxyz, fxyz]), np.concatenate([prgb, frgb]),
                            vr.StorageType.VOXEL_CLUSTER_STORE)
    cam = vr.Camera(view.world(view.eye), view.world(view.look_at), UP, view.fov, ASPECT)
    lit = vr.setup_constant_values()
    info = vr.VoxelSceneInfo(view.translation, view.scale)
    vr.forget_orders(torch.cuda.current_device())
    first, _ = gpu_render(scene, algo, cam, lit, info, CW, CH)
    for _ in range(39):
        got, _ = gpu_render(scene, algo, cam, lit, info, CW, CH)
        assert np.array_equal(got, first)
    scene.edit(fxyz, np.full(len(frgb), VOXEL_REMOVE, dtype=np.uint32))
    want, wbytes = points_frame(view_name, algo)
    for i in range(4):
        got, gbytes = gpu_render(scene, algo, cam, lit, info, CW, CH, count=True)
        assert np.array_equal(got, want), f"render {i + 1} after the edit: " + diff_report(got, want, CW)
        assert gbytes == wbytes, f"render {i + 1} after the edit: bytes gpu {gbytes} != oracle {wbytes}"
    scene.close()
