"""vr_pick on the GPU against the CPU reference (tests/pick_ref.py, itself held to the oracle
by tests/test_pick_ref.py): a pick reports exactly the hit the rendered pixel is shaded from
-- both stores, both algorithms, scaled and translated scenes, negative coordinates, walks
that crawl for 10^5..10^6 iterations, walks that never finish -- record by record, field by
field (`point` by its bits, any NaN equal to any NaN); and a pick leaves renders as they were."""
from __future__ import annotations

import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from tests import pick_ref, pyref
from tests.crawl_views import ASPECT, H as CH, LONG_WALK, MIN_LONG_PIXELS, SCENES, UP, VIEWS, W as CW
from tests.helpers import GOLDEN, gpu_render

pytestmark = pytest.mark.gpu

vr = pytest.importorskip("voxelraymarcher_amd")
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "voxelraymarcher_amd", "bin", "VoxelRaymarcher")

VCS, HASH = vr.StorageType.VOXEL_CLUSTER_STORE, vr.StorageType.HASH_TABLE
ORIGINAL, LONGEST = vr.RayMarchAlgorithm.ORIGINAL, vr.RayMarchAlgorithm.LONGEST_AXIS
PAIRS = [(s, a) for s in (VCS, HASH) for a in (ORIGINAL, LONGEST)]
PAIR_ID = lambda p: f"{p[0].name}-{p[1].name}"   # noqa: E731
LIGHT_POS = (40.0, 90.0, 30.0)


def golden_voxels():
    d = np.load(os.path.join(GOLDEN, "c1_scene.npz"))
    return d["xyz"], d["rgb"]


def frame_pixels(W, H):
    i = np.arange(W * H)
    return (i % W).astype(np.uint32), (i // W).astype(np.uint32)


def reference(xyz, rgb, store, algo, cam, W, H, px, py, scale, translation=(0.0, 0.0, 0.0)):
    ps = pyref.Scene(xyz, rgb, int(store))
    return pick_ref.pick_pixels(ps, cam, W, H, px, py, scale, algo == LONGEST, translation)


def assert_same(got, want, px, py, where=""):
    bad = pick_ref.same_records(got, want)
    assert bad.size == 0, (f"{where}: {bad.size} of {len(got)} records differ; first at pixel "
                           f"({int(px[bad[0]])}, {int(py[bad[0]])}): gpu {got[bad[0]]} reference {want[bad[0]]}")


# ---------------------------------------------------------------- 1. the golden C1 scene

@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_ID)
def test_golden_scene_every_pixel(pair):
    store, algo = pair
    xyz, rgb = golden_voxels()
    W, H, scale = 32, 24, 12
    cam = vr.Camera.reference(W, H)
    px, py = frame_pixels(W, H)
    with vr.create_scene(xyz, rgb, store) as scene:
        got = vr.pick(scene, algo, cam, vr.VoxelSceneInfo((0.0, 0.0, 0.0), scale), W, H, px, py)
    assert got.dtype == vr.HIT_DTYPE and got.shape == (W * H,)
    want, _ = reference(xyz, rgb, store, algo, cam, W, H, px, py, scale)
    assert_same(got, want, px, py)
    assert np.count_nonzero(got["status"] == vr.HitStatus.VOXEL) > 50
    assert np.count_nonzero(got["status"] == vr.HitStatus.MISS) > 50


# ---------------------------------------------------------------- 2. the frame from the records

@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_ID)
def test_render_is_the_shading_of_the_records(pair):
    """vr_render without shadows, under a point light (its shading reads the colour, the normal,
    the region and the point of the hit), equals applyLighting recomputed on the CPU from the
    pick records alone: 0 where the record is not VOXEL."""
    store, algo = pair
    xyz, rgb = golden_voxels()
    W, H, scale = 64, 48, 12
    cam = vr.Camera.reference(W, H)
    info = vr.VoxelSceneInfo((0.0, 0.0, 0.0), scale)
    lit = vr.setup_constant_values(use_shadows=False, use_point_light=True, light_position=LIGHT_POS)
    px, py = frame_pixels(W, H)
    with vr.create_scene(xyz, rgb, store) as scene:
        frame, _ = gpu_render(scene, algo, cam, lit, info, W, H)
        recs = scene.pick(algo, cam, info, W, H, px, py)
    ps = pyref.Scene(xyz, rgb, int(store))
    plit = pyref.Lighting(False, True, LIGHT_POS)
    want = np.array([pick_ref.shade(ps, r, plit) for r in recs], dtype=np.uint32)
    bad = np.flatnonzero(frame != want)
    assert bad.size == 0, (bad.size, int(bad[0]) % W, int(bad[0]) // W, hex(int(frame[bad[0]])), hex(int(want[bad[0]])))
    assert np.count_nonzero(frame) > 200


# ---------------------------------------------------------------- 3. batch shapes, 4. staging paths

def raw_pick(scene, algo, cam, info, W, H, px, py, n, hits, in_dev, out_dev):
    """vr_pick itself, on the caller's buffers (numpy arrays or CUDA tensors)."""
    ptr = lambda a: ctypes.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)   # noqa: E731
    vr._capi.check(vr.lib().vr_pick(scene.handle, int(algo), ctypes.byref(cam.raw), vr._capi.f3(info.translation),
                                    int(info.scale), W, H, ptr(px), ptr(py), n, int(in_dev), ptr(hits), int(out_dev),
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "vr_pick")


@pytest.fixture(scope="module")
def batch():
    """A shuffled pixel list of the golden frame with duplicates and pixels outside the frame,
    its scene and the records of the whole list in one call."""
    xyz, rgb = golden_voxels()
    W, H, scale = 32, 24, 12
    rng = np.random.default_rng(9)
    idx = rng.permutation(W * H)[:280]
    px, py = (idx % W).astype(np.uint32), (idx // W).astype(np.uint32)
    px[40], py[40] = px[3], py[3]                        # duplicates
    px[200], py[200] = px[3], py[3]
    for k, (x, y) in ((0, (W, 0)), (62, (0, H)), (64, (0xFFFFFFFF, 0xFFFFFFFF)), (130, (W, H)), (256, (5, H))):
        px[k], py[k] = x, y
    scene = vr.create_scene(xyz, rgb, VCS)
    cam = vr.Camera.reference(W, H)
    info = vr.VoxelSceneInfo((0.0, 0.0, 0.0), scale)
    full = vr.pick(scene, ORIGINAL, cam, info, W, H, px, py)
    yield dict(scene=scene, cam=cam, info=info, W=W, H=H, px=px, py=py, full=full, xyz=xyz, rgb=rgb)
    scene.close()


def test_batch_full_list_matches_reference(batch):
    b = batch
    want, _ = reference(b["xyz"], b["rgb"], VCS, ORIGINAL, b["cam"], b["W"], b["H"], b["px"], b["py"], b["info"].scale)
    assert_same(b["full"], want, b["px"], b["py"])
    out = b["full"][[0, 62, 64, 130, 256]]
    assert (out["status"] == vr.HitStatus.OUTSIDE).all()
    assert all(r.tobytes()[4:] == bytes(60) for r in out)
    assert b["full"][40].tobytes() == b["full"][3].tobytes() == b["full"][200].tobytes()
    assert np.count_nonzero(b["full"]["status"] == vr.HitStatus.VOXEL) > 20


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257])
def test_batch_prefix_and_sentinel(batch, n):
    """n queries give the first n records of the full call -- the OUTSIDE entries' wave
    neighbours included -- and record n of an n + 1 record buffer is never written."""
    b = batch
    hits = np.full(n + 1, 0xAB, dtype=np.uint8).repeat(64).view(vr.HIT_DTYPE)
    raw_pick(b["scene"], ORIGINAL, b["cam"], b["info"], b["W"], b["H"], b["px"], b["py"], n, hits, False, False)
    assert hits[:n].tobytes() == b["full"][:n].tobytes()
    assert hits[n].tobytes() == bytes([0xAB]) * 64
    dpx = torch.from_numpy(b["px"].view(np.int32)).cuda()
    dpy = torch.from_numpy(b["py"].view(np.int32)).cuda()
    dh = torch.full((n + 1, 16), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    raw_pick(b["scene"], ORIGINAL, b["cam"], b["info"], b["W"], b["H"], dpx, dpy, n, dh, True, True)
    got = dh.cpu().numpy()
    assert got[:n].tobytes() == b["full"][:n].tobytes()
    assert (got[n] == 0x5A5A5A5A).all()


def test_host_and_device_paths_give_the_same_bytes(batch):
    b = batch
    n = len(b["px"])
    dpx = torch.from_numpy(b["px"].view(np.int32)).cuda()
    dpy = torch.from_numpy(b["py"].view(np.int32)).cuda()
    for in_dev in (False, True):
        for out_dev in (False, True):
            hits = torch.zeros((n, 16), dtype=torch.int32, device="cuda") if out_dev else np.zeros(n, dtype=vr.HIT_DTYPE)
            raw_pick(b["scene"], ORIGINAL, b["cam"], b["info"], b["W"], b["H"], dpx if in_dev else b["px"],
                     dpy if in_dev else b["py"], n, hits, in_dev, out_dev)
            got = hits.cpu().numpy() if out_dev else hits
            assert got.tobytes() == b["full"].tobytes(), (in_dev, out_dev)
    # the package's tensor form: (n, 16) int32 of the same bytes
    t = vr.pick(b["scene"], ORIGINAL, b["cam"], b["info"], b["W"], b["H"], dpx, dpy)
    assert t.is_cuda and t.dtype == torch.int32 and tuple(t.shape) == (n, 16)
    assert t.cpu().numpy().tobytes() == b["full"].tobytes()
    assert len(vr.pick(b["scene"], ORIGINAL, b["cam"], b["info"], b["W"], b["H"], [], [])) == 0


def test_pick_refuses_graph_capture(batch):
    """vr_pick on a stream that is capturing a graph returns VR_E_INVALID before it enqueues or
    allocates anything (the call ends in a stream synchronise, which a capture cannot hold); the
    capture ends cleanly and a pick after it is exact.  (As test_render_refuses_graph_capture.)"""
    b = batch
    n = len(b["px"])
    dpx = torch.from_numpy(b["px"].view(np.int32)).cuda()
    dpy = torch.from_numpy(b["py"].view(np.int32)).cuda()
    dh = torch.zeros((n, 16), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    err = None
    with torch.cuda.graph(g, stream=s):
        try:
            raw_pick(b["scene"], ORIGINAL, b["cam"], b["info"], b["W"], b["H"], dpx, dpy, n, dh, True, True)
        except vr.VrError as e:
            err = e
    assert err is not None and err.code == -1 and "captur" in str(err) and "vr_pick" in str(err)
    torch.cuda.synchronize()
    assert not dh.any()
    raw_pick(b["scene"], ORIGINAL, b["cam"], b["info"], b["W"], b["H"], dpx, dpy, n, dh, True, True)
    assert dh.cpu().numpy().tobytes() == b["full"].tobytes()


# ---------------------------------------------------------------- 5. negative coordinates, translated

@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_ID)
def test_negative_coordinates_and_translation(pair):
    """The scene, translation and camera of test_oracle_matches_python_restatement_negative_and_translated."""
    store, algo = pair
    rng = np.random.default_rng(5)
    xyz = rng.integers(-80, 70, size=(2500, 3)).astype(np.int32)
    rgb = rng.integers(0, 1 << 24, size=2500).astype(np.uint32)
    cam = vr.Camera((90.0, 40.0, 100.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 70.0, 4.0 / 3.0)
    tr = (-1.0, -0.5, 0.25)
    W, H = 160, 120
    idx = np.random.default_rng(55).permutation(W * H)[:200]
    px, py = (idx % W).astype(np.uint32), (idx // W).astype(np.uint32)
    with vr.create_scene(xyz, rgb, store) as scene:
        got = vr.pick(scene, algo, cam, vr.VoxelSceneInfo(tr, 1), W, H, px, py)
    want, _ = reference(xyz, rgb, store, algo, cam, W, H, px, py, 1, tr)
    assert_same(got, want, px, py)
    hit = got[got["status"] == vr.HitStatus.VOXEL]
    assert len(hit) > 10 and (hit["voxel"] < 0).any() and (hit["region"] < 0).any()


# ---------------------------------------------------------------- 6. crawl views

@pytest.mark.parametrize("pair", [(VCS, ORIGINAL), (VCS, LONGEST), (HASH, ORIGINAL)], ids=PAIR_ID)
@pytest.mark.parametrize("name", ["y-plane", "z-plane", "y-plane-scale2"])
def test_crawl_views(name, pair):
    """Primary walks that crawl for 65 536 to ~10^6 iterations (tests/crawl_views.py): the pick's
    exact walker fast-forwards them.  The cluster store: every pixel; the hash table (no
    clusters, no crawls) sampled."""
    store, algo = pair
    view = {v.name: v for v in VIEWS}[name]
    xyz, rgb = SCENES[view.scene]()
    cam = vr.Camera(view.world(view.eye), view.world(view.look_at), UP, view.fov, ASPECT)
    px, py = frame_pixels(CW, CH)
    if store == HASH:
        idx = np.random.default_rng(21).permutation(CW * CH)[:256]
        px, py = px[idx], py[idx]
    with vr.create_scene(xyz, rgb, store) as scene:
        got = vr.pick(scene, algo, cam, vr.VoxelSceneInfo(view.translation, view.scale), CW, CH, px, py)
    want, iters = reference(xyz, rgb, store, algo, cam, CW, CH, px, py, view.scale, view.translation)
    assert_same(got, want, px, py, name)
    if store == VCS:
        assert int(np.count_nonzero(iters >= LONG_WALK)) >= MIN_LONG_PIXELS[False]


# ---------------------------------------------------------------- 7. the aliasing fixture

def test_alias_rays_invent_no_voxel():
    """tests/golden/alias_rays.json: longest-axis walks of the cluster store that probe outside
    their region where the `short` cluster id aliases into the directory.  The aliased probe
    path must keep answering "no voxel": the records equal the reference's."""
    fx = json.load(open(os.path.join(GOLDEN, "alias_rays.json")))
    d = np.load(os.path.join(GOLDEN, fx["scene"]))
    W, H = fx["width"], fx["height"]
    px, py = frame_pixels(W, H)
    ps = pyref.Scene(d["xyz"], d["rgb"], 0)
    stored = set(map(tuple, d["xyz"].tolist()))
    with vr.create_scene(d["xyz"], d["rgb"], VCS) as scene:
        for c in fx["cameras"][:20]:
            cam = vr.Camera(c["eye"], c["at"], fx["up"], fx["fov"], fx["aspect"])
            got = vr.pick(scene, LONGEST, cam, vr.VoxelSceneInfo((0.0, 0.0, 0.0), fx["scale"]), W, H, px, py)
            want, _ = pick_ref.pick_pixels(ps, cam, W, H, px, py, fx["scale"], True)
            assert_same(got, want, px, py, str(c["eye"]))
            for r in got[got["status"] == vr.HitStatus.VOXEL]:
                assert tuple(int(v) for v in r["voxel"]) in stored


# ---------------------------------------------------------------- 8. walks that never finish

def nan_camera():
    """tests/test_oracle.py nan_camera as a vr.Camera: every ray's direction is NaN."""
    cam = vr.Camera.reference(4, 4)
    for i in range(3):
        cam.raw.origin[i] = cam.raw.lower_left[i] = 1.0
        cam.raw.horizontal[i] = cam.raw.vertical[i] = cam.raw.forward[i] = 0.0
    return cam


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_ID)
def test_never_finishing_walks(pair):
    """4x4, scale 12: the original walks never finish (NEVER, every other field 0); the
    longest-axis walks end in a voxel with a NaN hit point, as the reference's do."""
    store, algo = pair
    xyz, rgb = golden_voxels()
    cam = nan_camera()
    px, py = frame_pixels(4, 4)
    with vr.create_scene(xyz, rgb, store) as scene:
        got = vr.pick(scene, algo, cam, vr.VoxelSceneInfo((0.0, 0.0, 0.0), 12), 4, 4, px, py)
    want, _ = reference(xyz, rgb, store, algo, cam, 4, 4, px, py, 12)
    assert_same(got, want, px, py)
    if algo == ORIGINAL:
        assert (got["status"] == vr.HitStatus.NEVER).all() and all(r.tobytes()[4:] == bytes(60) for r in got)
    else:
        assert (got["status"] == vr.HitStatus.VOXEL).all() and np.isnan(got["point"]).all()


# ---------------------------------------------------------------- 9. pick, edit, pick

@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_ID)
def test_pick_edit_pick(pair):
    store, algo = pair
    xyz, rgb = golden_voxels()
    W, H, scale = 32, 24, 12
    cam = vr.Camera.reference(W, H)
    info = vr.VoxelSceneInfo((0.0, 0.0, 0.0), scale)
    px, py = np.array([W // 2], np.uint32), np.array([H // 2], np.uint32)
    voxels = {tuple(p): int(c) for p, c in zip(xyz.tolist(), rgb.tolist())}

    def ref_now():
        k = np.array(list(voxels.keys()), np.int32)
        v = np.array(list(voxels.values()), np.uint32)
        return reference(k, v, store, algo, cam, W, H, px, py, scale)[0]

    with vr.create_scene(xyz, rgb, store) as scene:
        first = scene.pick(algo, cam, info, W, H, px, py)
        assert_same(first, ref_now(), px, py, "before the edit")
        assert int(first[0]["status"]) == vr.HitStatus.VOXEL
        v0 = tuple(int(c) for c in first[0]["voxel"])
        assert voxels[v0] == int(first[0]["color"])
        scene.edit(np.array([v0], np.int32), np.array([vr.VOXEL_REMOVE], np.uint32))
        del voxels[v0]
        second = scene.pick(algo, cam, info, W, H, px, py)
        assert_same(second, ref_now(), px, py, "after the removal")
        assert tuple(int(c) for c in second[0]["voxel"]) != v0 or int(second[0]["status"]) != vr.HitStatus.VOXEL
        if int(second[0]["status"]) == vr.HitStatus.VOXEL:
            cell = tuple(int(a) + int(b) for a, b in zip(second[0]["voxel"], second[0]["normal"]))
            if all(0 <= c < 64 for c in cell) and cell not in voxels:      # (the scene's frame: one region)
                scene.edit(np.array([cell], np.int32), np.array([0x00ABCDEF], np.uint32))
                voxels[cell] = 0x00ABCDEF
                assert_same(scene.pick(algo, cam, info, W, H, px, py), ref_now(), px, py, "after the insertion")
        xyz_now, rgb_now = scene.voxels()
        assert {tuple(p): int(c) for p, c in zip(xyz_now.tolist(), rgb_now.tolist())} == voxels


# ---------------------------------------------------------------- 10. renders undisturbed

def test_pick_leaves_renders_alone():
    """A view that defers crawling pixels, rendered until its orders and crawl state are learned;
    then 100 picks; then the same frame again, from a plain render and from a PreparedRender."""
    view = {v.name: v for v in VIEWS}["y-plane"]
    xyz, rgb = SCENES[view.scene]()
    cam = vr.Camera(view.world(view.eye), view.world(view.look_at), UP, view.fov, ASPECT)
    # (a point light at the eye: under the default light every hit of this view faces away)
    lit = vr.setup_constant_values(use_point_light=True, light_position=view.world(view.eye))
    info = vr.VoxelSceneInfo(view.translation, view.scale)
    idx = np.random.default_rng(3).permutation(CW * CH)[:100]
    px, py = (idx % CW).astype(np.uint32), (idx // CW).astype(np.uint32)
    allx, ally = frame_pixels(CW, CH)
    with vr.create_scene(xyz, rgb, VCS) as scene:
        frames = [gpu_render(scene, ORIGINAL, cam, lit, info, CW, CH)[0] for _ in range(3)]
        uses = vr.debug_order_uses(0)
        recs = vr.pick(scene, ORIGINAL, cam, info, CW, CH, px, py)
        assert vr.debug_order_uses(0) == uses      # (not a render launch: none of the eight values moves)
        frames.append(gpu_render(scene, ORIGINAL, cam, lit, info, CW, CH)[0])
        prep = vr.PreparedRender(scene, ORIGINAL, cam, lit, info, CW, CH)
        out = torch.full((CW * CH,), -1, dtype=torch.int32, device="cuda")
        prep(out)
        recs2 = vr.pick(scene, ORIGINAL, cam, info, CW, CH, px, py)
        prep(out)
        torch.cuda.synchronize()
        frames.append(out.cpu().numpy().view(np.uint32))
        uses = vr.debug_order_uses(0)
        every = vr.pick(scene, ORIGINAL, cam, info, CW, CH, allx, ally)
        assert vr.debug_order_uses(0) == uses and uses["launches"] >= 6
    for f in frames[1:]:
        assert np.array_equal(f, frames[0])
    assert np.count_nonzero(frames[0]) >= 10
    assert recs.tobytes() == recs2.tobytes() == every[idx].tobytes()
    # a lit pixel has a hit behind it (a pixel that is 0 may have one too: unlit or shadowed)
    assert (every["status"][frames[0] != 0] == vr.HitStatus.VOXEL).all()


# ---------------------------------------------------------------- 11. the CLI

def pick_line(x, y, r):
    if int(r["status"]) == vr.HitStatus.VOXEL:
        v, n = r["voxel"], r["normal"]
        return f"pick {x} {y} voxel {v[0]} {v[1]} {v[2]} color 0x{int(r['color']):06X} normal {n[0]} {n[1]} {n[2]}"
    return f"pick {x} {y} " + {0: "miss", 2: "never", 3: "outside"}[int(r["status"])]


@pytest.mark.parametrize("store,algo", [("vcs", "original"), ("hashtable", "longestaxis")])
def test_cli_pick(tmp_path, store, algo):
    """`VoxelRaymarcher ... --pick X,Y` (repeated) prints, after the frame is rendered, the line
    the Python pick gives for each pixel."""
    xyz, rgb = golden_voxels()
    scene_path = str(tmp_path / "scene.vox")
    vr.write_voxel_file(scene_path, xyz, rgb)
    W, H, scale = 96, 64, 12
    picks = [(48, 32), (10, 50), (0, 0), (95, 63), (96, 0), (70, 20), (48, 32)]
    out = str(tmp_path / "output.png")
    args = [EXE, str(scale), store, algo, "--scene", scene_path, "--width", str(W), "--height", str(H), "--out", out]
    for x, y in picks:
        args += ["--pick", f"{x},{y}"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    got = [ln for ln in lines if ln.startswith("pick ")]
    with vr.create_scene(xyz, rgb, vr.parse_storage(store)) as scene:
        recs = vr.pick(scene, vr.parse_algorithm(algo), vr.Camera.reference(W, H), vr.VoxelSceneInfo((0.0, 0.0, 0.0), scale),
                       W, H, [p[0] for p in picks], [p[1] for p in picks])
    assert got == [pick_line(x, y, rec) for (x, y), rec in zip(picks, recs)]
    assert any(" voxel " in ln for ln in got) and got[4] == "pick 96 0 outside"
    # after the render, before the image is written
    order = [i for i, ln in enumerate(lines) if ln.startswith(("Execution Time", "pick ", "Wrote "))]
    assert [lines[i].split()[0] for i in order] == ["Execution"] + ["pick"] * len(picks) + ["Wrote"]
    assert os.path.exists(out)


def test_cli_pick_refused_with_several_gpus(tmp_path):
    r = subprocess.run([EXE, "1", "vcs", "original", "--synth", "64", "--width", "64", "--height", "64", "--out",
                        str(tmp_path / "o.png"), "--gpus", "2", "--pick", "1,1"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "--pick" in r.stderr, r.stdout + r.stderr
    assert not os.path.exists(tmp_path / "o.png")
    r = subprocess.run([EXE, "1", "vcs", "original", "--pick", "3;4"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--pick needs X,Y" in r.stderr
