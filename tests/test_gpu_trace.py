"""vr_trace and vr_camera_rays on the GPU against the CPU reference (tests/trace_ref.py, tied to
the pick reference and through it to the oracle by tests/test_trace_ref.py): a trace reports,
for any ray, exactly the record the reference's primary walk gives -- both stores, both
algorithms, every execution order, scaled and translated scenes over several regions, rays no
caller should send -- record by record, field by field (`point` by its bits, any NaN equal to
any NaN); trace(camera_rays(pixels)) is pick(pixels) byte for byte; and a trace leaves renders
as they were."""
from __future__ import annotations

import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import fuzz_cases, pick_ref, pyref, trace_cases, trace_ref
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
ORDERS = [vr.TraceOrder.GIVEN, vr.TraceOrder.COHERENT, vr.TraceOrder.AUTO]
ZERO = (0.0, 0.0, 0.0)


def golden_voxels():
    d = np.load(os.path.join(GOLDEN, "c1_scene.npz"))
    return d["xyz"], d["rgb"]


def frame_pixels(W, H):
    i = np.arange(W * H)
    return (i % W).astype(np.uint32), (i // W).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def golden_rays():
    """The 256 seeded rays of tests 2, 5 and 6 (never modified: callers copy)."""
    rays = trace_cases.random_rays(golden_voxels()[0], seed=11)
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def golden_reference(store, algo):
    """The reference's records of golden_rays() at scale 1, computed once per pair."""
    xyz, rgb = golden_voxels()
    recs, iters = trace_ref.trace_rays(pyref.Scene(xyz, rgb, int(store)), golden_rays(), 1, algo == LONGEST)
    recs.setflags(write=False)
    return recs, iters


def assert_same(got, want, where=""):
    bad = pick_ref.same_records(got, want)
    assert bad.size == 0, (f"{where}: {bad.size} of {len(got)} records differ; first at ray {int(bad[0])}: "
                           f"gpu {got[bad[0]]} reference {want[bad[0]]}")


# ---------------------------------------------------------------- 1. identity with pick

@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_ID)
def test_trace_of_camera_rays_is_pick(pair):
    store, algo = pair
    xyz, rgb = golden_voxels()
    W, H, scale = 32, 24, 12
    cam = vr.Camera.reference(W, H)
    info = vr.VoxelSceneInfo(ZERO, scale)
    px, py = frame_pixels(W, H)
    rays = vr.camera_rays(cam, W, H, px, py)
    assert rays.dtype == vr.RAY_DTYPE and rays.shape == (W * H,)
    assert rays.tobytes() == trace_ref.camera_rays(cam, W, H, px, py).tobytes()
    with vr.create_scene(xyz, rgb, store) as scene:
        want = vr.pick(scene, algo, cam, info, W, H, px, py)
        for order in ORDERS:
            got = scene.trace(algo, info, rays, order=order)
            assert got.dtype == vr.HIT_DTYPE and got.tobytes() == want.tobytes(), order
        # the tensor forms: (n, 8) float32 rays of the same bytes in, (n, 16) int32 records out
        dpx, dpy = (torch.from_numpy(a.view(np.int32)).cuda() for a in (px, py))
        drays = vr.camera_rays(cam, W, H, dpx, dpy)
        assert drays.is_cuda and drays.dtype == torch.float32 and tuple(drays.shape) == (W * H, 8)
        assert drays.cpu().numpy().tobytes() == rays.tobytes()
        dhits = vr.trace(scene, algo, info, drays)
        assert dhits.is_cuda and dhits.dtype == torch.int32 and tuple(dhits.shape) == (W * H, 16)
        assert dhits.cpu().numpy().tobytes() == want.tobytes()
    assert np.count_nonzero(want["status"] == vr.HitStatus.VOXEL) > 50
    assert np.count_nonzero(want["status"] == vr.HitStatus.MISS) > 50


def test_camera_rays_outside_the_frame_are_nan():
    W, H = 32, 24
    cam = vr.Camera.reference(W, H)
    px = np.array([W, 0, 0xFFFFFFFF, W, 5, 3], np.uint32)
    py = np.array([0, H, 0xFFFFFFFF, H, H, 2], np.uint32)
    rays = vr.camera_rays(cam, W, H, px, py)
    nan_ray = np.array([0x7FC00000] * 3 + [0], dtype=np.uint32).tobytes() * 2
    assert all(r.tobytes() == nan_ray for r in rays[:5])
    assert rays[5].tobytes() == trace_ref.camera_ray(cam, W, H, 3, 2).tobytes() and np.isfinite(rays[5]["origin"]).all()
    assert len(vr.camera_rays(cam, W, H, [], [])) == 0


# ---------------------------------------------------------------- 2. arbitrary rays

@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_ID)
def test_arbitrary_rays_match_reference_under_every_order(pair):
    store, algo = pair
    xyz, rgb = golden_voxels()
    rays = golden_rays()
    want, iters = golden_reference(store, algo)
    # the yardstick itself: an all-miss (or all-hit) kernel cannot pass
    assert np.count_nonzero(want["status"] == trace_ref.VOXEL) >= 20
    assert np.count_nonzero(want["status"] == trace_ref.MISS) >= 20
    length = np.linalg.norm(rays["direction"].astype(np.float64), axis=1)
    assert length.min() < 0.01 and length.max() > 100.0 and np.count_nonzero(rays["direction"] == 0.0) >= 20
    info = vr.VoxelSceneInfo(ZERO, 1)
    with vr.create_scene(xyz, rgb, store) as scene:
        for order in ORDERS:
            assert_same(vr.trace(scene, algo, info, rays, order=order), want, order.name)
        # the (n, 6) form: origin, direction
        flat = np.concatenate([rays["origin"], rays["direction"]], axis=1)
        assert vr.trace(scene, algo, info, flat, order=vr.TraceOrder.GIVEN).tobytes() == \
            vr.trace(scene, algo, info, rays, order=vr.TraceOrder.GIVEN).tobytes()
        assert len(vr.trace(scene, algo, info, np.zeros(0, vr.RAY_DTYPE))) == 0


# ---------------------------------------------------------------- 3. several regions

@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_ID)
def test_several_regions_negative_coordinates_translated_scaled(pair):
    """tests/fuzz_cases.py make_wide_case(81): voxels from (-122, -248, -192) to (77, -49, 6) over
    several 64^3 regions, scale 2, translation (-3.5, 4.5, -6.5)."""
    store, algo = pair
    c = fuzz_cases.make_wide_case(81)
    assert c.scale == 2 and c.translation == (-3.5, 4.5, -6.5) and c.xyz.min() < -64 and np.ptp(c.xyz, axis=0).min() > 128
    rays = trace_cases.random_rays(c.xyz, seed=12, scale=c.scale, translation=c.translation)
    want, _ = trace_ref.trace_rays(pyref.Scene(c.xyz, c.rgb, int(store)), rays, c.scale, algo == LONGEST, c.translation)
    assert np.count_nonzero(want["status"] == trace_ref.VOXEL) >= 20
    assert np.count_nonzero(want["status"] == trace_ref.MISS) >= 20
    info = vr.VoxelSceneInfo(c.translation, c.scale)
    with vr.create_scene(c.xyz, c.rgb, store) as scene:
        for order in ORDERS:
            got = vr.trace(scene, algo, info, rays, order=order)
            assert_same(got, want, order.name)
    hit = got[got["status"] == vr.HitStatus.VOXEL]
    assert (hit["voxel"] < 0).any() and (hit["region"] < 0).any() and len(np.unique(hit["region"], axis=0)) > 1


# ---------------------------------------------------------------- 4. degenerate rays

def test_degenerate_rays_get_the_reference_record():
    """Zero, NaN and infinite directions and origins, an origin at -3e9, a direction of 1e-30,
    axis-aligned rays: no ray is rejected and each record is the reference's, whatever it is."""
    xyz, rgb = golden_voxels()
    names, rays = trace_cases.degenerate_rays(inside=(30.5, 40.25, 20.75), outside=(-50.0, 100.0, 30.0))
    info = vr.VoxelSceneInfo(ZERO, 1)
    seen = {}
    for store, algo in PAIRS:
        want, _ = trace_ref.trace_rays(pyref.Scene(xyz, rgb, int(store)), rays, 1, algo == LONGEST)
        with vr.create_scene(xyz, rgb, store) as scene:
            for order in (vr.TraceOrder.GIVEN, vr.TraceOrder.COHERENT):
                got = vr.trace(scene, algo, info, rays, order=order)
                bad = pick_ref.same_records(got, want)
                assert bad.size == 0, (store, algo, order, [names[i] for i in bad], got[bad[:1]], want[bad[:1]])
        assert not (got["status"] == vr.HitStatus.OUTSIDE).any()
        for r in got[got["status"] != vr.HitStatus.VOXEL]:
            assert r.tobytes()[4:] == bytes(60)
        seen[(store, algo)] = dict(zip(names, got["status"].tolist()))
    # a zero direction normalises to NaN: from inside the scene the original walk never finishes
    for store in (VCS, HASH):
        assert seen[(store, ORIGINAL)]["zero direction, inside"] == vr.HitStatus.NEVER
    assert any(vr.HitStatus.VOXEL in s.values() for s in seen.values())
    assert any(vr.HitStatus.MISS in s.values() for s in seen.values())


# ---------------------------------------------------------------- 5. batch edges

def raw_trace(scene, algo, info, rays, n, hits, in_dev, out_dev, order):
    """vr_trace itself, on the caller's buffers (numpy arrays or CUDA tensors)."""
    ptr = lambda a: ctypes.c_void_p(a if isinstance(a, int) else (a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data))   # noqa: E731
    vr._capi.check(vr.lib().vr_trace(scene.handle, int(algo), vr._capi.f3(info.translation), int(info.scale), ptr(rays), n,
                                     int(in_dev), ptr(hits), int(out_dev), int(order),
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "vr_trace")


@pytest.fixture(scope="module")
def batch():
    """The golden rays with duplicates (258 rays), their scene and the records of one full call."""
    xyz, rgb = golden_voxels()
    rays = np.concatenate([golden_rays(), golden_rays()[[3, 100]]])
    rays[40] = rays[3]
    rays[200] = rays[3]
    scene = vr.create_scene(xyz, rgb, VCS)
    info = vr.VoxelSceneInfo(ZERO, 1)
    full = vr.trace(scene, ORIGINAL, info, rays, order=vr.TraceOrder.GIVEN)
    drays = torch.from_numpy(rays.view(np.float32).reshape(-1, 8)).cuda()
    yield dict(scene=scene, info=info, rays=rays, drays=drays, full=full)
    scene.close()


def test_batch_full_list(batch):
    b = batch
    want, _ = golden_reference(VCS, ORIGINAL)
    assert_same(b["full"][:256][[i for i in range(256) if i not in (40, 200)]],
                want[[i for i in range(256) if i not in (40, 200)]])
    assert b["full"][40].tobytes() == b["full"][3].tobytes() == b["full"][200].tobytes() == b["full"][256].tobytes()
    assert b["full"][257].tobytes() == b["full"][100].tobytes()


@pytest.mark.parametrize("order", [vr.TraceOrder.GIVEN, vr.TraceOrder.COHERENT], ids=lambda o: o.name)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257])
def test_batch_prefix_and_sentinel(batch, n, order):
    """n rays give the first n records of the full call, and record n of an n + 1 record buffer
    is never written: on host buffers and on device buffers."""
    b = batch
    hits = np.full(n + 1, 0xAB, dtype=np.uint8).repeat(64).view(vr.HIT_DTYPE)
    raw_trace(b["scene"], ORIGINAL, b["info"], b["rays"], n, hits, False, False, order)
    assert hits[:n].tobytes() == b["full"][:n].tobytes()
    assert hits[n].tobytes() == bytes([0xAB]) * 64
    dh = torch.full((n + 1, 16), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    raw_trace(b["scene"], ORIGINAL, b["info"], b["drays"], n, dh, True, True, order)
    got = dh.cpu().numpy()
    assert got[:n].tobytes() == b["full"][:n].tobytes()
    assert (got[n] == 0x5A5A5A5A).all()
    # the mixed forms: device rays to host records, host rays to device records
    hits = np.full(n + 1, 0xAB, dtype=np.uint8).repeat(64).view(vr.HIT_DTYPE)
    raw_trace(b["scene"], ORIGINAL, b["info"], b["drays"], n, hits, True, False, order)
    assert hits[:n].tobytes() == b["full"][:n].tobytes()
    assert hits[n].tobytes() == bytes([0xAB]) * 64
    dh = torch.full((n + 1, 16), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    raw_trace(b["scene"], ORIGINAL, b["info"], b["rays"], n, dh, False, True, order)
    got = dh.cpu().numpy()
    assert got[:n].tobytes() == b["full"][:n].tobytes()
    assert (got[n] == 0x5A5A5A5A).all()


@pytest.mark.parametrize("n", [1, 257])
def test_camera_rays_every_staging_mode(n):
    """vr_camera_rays with its pixels and its rays each on the host or on the device: all four
    forms give the bytes of the host/host call for n pixels of the 32 x 24 golden frame, and
    record n of an n + 1 record buffer is never written."""
    W, H = 32, 24
    cam = vr.Camera.reference(W, H)
    px, py = (a[:n].copy() for a in frame_pixels(W, H))
    dpx, dpy = (torch.from_numpy(a.view(np.int32)).cuda() for a in (px, py))
    want = vr.camera_rays(cam, W, H, px, py)
    assert want.tobytes() == trace_ref.camera_rays(cam, W, H, px, py).tobytes()
    ptr = lambda a: ctypes.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)   # noqa: E731
    for in_dev in (False, True):
        for out_dev in (False, True):
            if out_dev:
                rays = torch.full((n + 1, 8), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            else:
                rays = np.full(n + 1, 0xAB, dtype=np.uint8).repeat(32).view(vr.RAY_DTYPE)
            qx, qy = (dpx, dpy) if in_dev else (px, py)
            vr._capi.check(vr.lib().vr_camera_rays(0, ctypes.byref(cam.raw), W, H, ptr(qx), ptr(qy), n, int(in_dev),
                                                   ptr(rays), int(out_dev),
                                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
                           "vr_camera_rays")
            got = rays.cpu().numpy() if out_dev else rays
            assert got[:n].tobytes() == want.tobytes(), (in_dev, out_dev)
            assert got[n].tobytes() == (bytes([0x5A]) if out_dev else bytes([0xAB])) * 32, (in_dev, out_dev)


# ---------------------------------------------------------------- 6. orders agree

def test_orders_agree_and_bad_buffers_are_refused(batch):
    """1000 shuffled rays (the golden rays repeated: repeated keys, four workgroups, a partial
    last wave): every order returns the same bytes, each record the reference's."""
    b = batch
    idx = np.random.default_rng(6).permutation(np.arange(1000) % 256)
    rays = golden_rays()[idx]
    want, _ = golden_reference(VCS, ORIGINAL)
    given = vr.trace(b["scene"], ORIGINAL, b["info"], rays, order=vr.TraceOrder.GIVEN)
    assert_same(given, want[idx])
    drays = torch.from_numpy(rays.view(np.float32).reshape(-1, 8)).cuda()
    for order in ORDERS:
        assert vr.trace(b["scene"], ORIGINAL, b["info"], rays, order=order).tobytes() == given.tobytes(), order
        assert vr.trace(b["scene"], ORIGINAL, b["info"], drays, order=order).cpu().numpy().tobytes() == given.tobytes(), order
    # a misaligned device pointer: refused, nothing written
    n = 64
    dh = torch.zeros((n + 1, 16), dtype=torch.int32, device="cuda")
    for bad_rays, bad_hits in ((drays.data_ptr() + 4, dh), (drays, dh.data_ptr() + 8)):
        with pytest.raises(vr.VrError) as e:
            raw_trace(b["scene"], ORIGINAL, b["info"], bad_rays, n, bad_hits, True, True, vr.TraceOrder.GIVEN)
        assert e.value.code == -1 and "vr_trace" in str(e.value) and "aligned" in str(e.value)
    torch.cuda.synchronize()
    assert not dh.any()


def test_trace_refuses_graph_capture(batch):
    """vr_trace and vr_camera_rays on a stream that is capturing a graph return VR_E_INVALID before
    they enqueue or allocate anything; the capture ends cleanly and a trace after it is exact.
    (As test_pick_refuses_graph_capture.)"""
    b = batch
    n = len(b["rays"])
    dh = torch.zeros((n, 16), dtype=torch.int32, device="cuda")
    cam = vr.Camera.reference(8, 8)
    dp = torch.zeros(4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    errs = []
    with torch.cuda.graph(g, stream=s):
        for order in (vr.TraceOrder.GIVEN, vr.TraceOrder.COHERENT):
            try:
                raw_trace(b["scene"], ORIGINAL, b["info"], b["drays"], n, dh, True, True, order)
            except vr.VrError as e:
                errs.append(e)
        try:
            vr.camera_rays(cam, 8, 8, dp, dp)
        except vr.VrError as e:
            errs.append(e)
    assert len(errs) == 3 and all(e.code == -1 and "captur" in str(e) for e in errs)
    assert "vr_trace" in str(errs[0]) and "vr_trace" in str(errs[1]) and "vr_camera_rays" in str(errs[2])
    torch.cuda.synchronize()
    assert not dh.any()
    raw_trace(b["scene"], ORIGINAL, b["info"], b["drays"], n, dh, True, True, vr.TraceOrder.COHERENT)
    assert dh.cpu().numpy().tobytes() == b["full"].tobytes()


# ---------------------------------------------------------------- 7. renders undisturbed

def test_trace_leaves_renders_alone():
    xyz, rgb = golden_voxels()
    W, H, scale = 64, 48, 12
    cam = vr.Camera.reference(W, H)
    info = vr.VoxelSceneInfo(ZERO, scale)
    lit = vr.setup_constant_values()
    px, py = frame_pixels(W, H)
    rays = vr.camera_rays(cam, W, H, px, py)
    with vr.create_scene(xyz, rgb, VCS) as scene:
        frames = [gpu_render(scene, ORIGINAL, cam, lit, info, W, H)[0] for _ in range(3)]
        uses = vr.debug_order_uses(0)
        recs = [vr.trace(scene, ORIGINAL, info, rays, order=order) for order in ORDERS]
        assert vr.debug_order_uses(0) == uses      # (not a render launch: none of the eight values moves)
        frames.append(gpu_render(scene, ORIGINAL, cam, lit, info, W, H)[0])
        assert vr.debug_order_uses(0)["launches"] == uses["launches"] + 1
    for f in frames[1:]:
        assert np.array_equal(f, frames[0])
    assert np.count_nonzero(frames[0]) > 200
    assert recs[0].tobytes() == recs[1].tobytes() == recs[2].tobytes()
    # a lit pixel has a hit behind it
    assert (recs[0]["status"][frames[0] != 0] == vr.HitStatus.VOXEL).all()


# ---------------------------------------------------------------- 8. trace, edit, trace

@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_ID)
def test_trace_edit_trace(pair):
    store, algo = pair
    xyz, rgb = golden_voxels()
    info = vr.VoxelSceneInfo(ZERO, 1)
    want, _ = golden_reference(store, algo)
    k = int(np.flatnonzero(want["status"] == trace_ref.VOXEL)[0])
    ray = golden_rays()[k:k + 1].copy()
    voxels = {tuple(p): int(c) for p, c in zip(xyz.tolist(), rgb.tolist())}
    with vr.create_scene(xyz, rgb, store) as scene:
        first = scene.trace(algo, info, ray)
        assert_same(first, want[k:k + 1], "before the edit")
        v0 = tuple(int(c) for c in first[0]["voxel"])
        assert voxels[v0] == int(first[0]["color"])
        scene.edit(np.array([v0], np.int32), np.array([vr.VOXEL_REMOVE], np.uint32))
        del voxels[v0]
        second = scene.trace(algo, info, ray)
    kk, vv = np.array(list(voxels.keys()), np.int32), np.array(list(voxels.values()), np.uint32)
    after, _ = trace_ref.trace_rays(pyref.Scene(kk, vv, int(store)), ray, 1, algo == LONGEST)
    assert_same(second, after, "after the removal")
    assert tuple(int(c) for c in second[0]["voxel"]) != v0 or int(second[0]["status"]) != vr.HitStatus.VOXEL


# ---------------------------------------------------------------- 9. the CLI

def g9(x):
    """printf's %.9g (which, unlike Python's format, prints a NaN's sign: "-nan")."""
    x = float(x)
    return ("-nan" if np.signbit(x) else "nan") if np.isnan(x) else f"{x:.9g}"


def trace_line(i, r):
    if int(r["status"]) == vr.HitStatus.VOXEL:
        v, n, p = r["voxel"], r["normal"], r["point"]
        return (f"trace {i} voxel {v[0]} {v[1]} {v[2]} color 0x{int(r['color']):06X} normal {n[0]} {n[1]} {n[2]} "
                f"point {g9(p[0])} {g9(p[1])} {g9(p[2])}")
    return f"trace {i} " + {0: "miss", 2: "never"}[int(r["status"])]


@pytest.mark.parametrize("store,algo", [("vcs", "original"), ("hashtable", "longestaxis")])
def test_cli_trace(tmp_path, store, algo):
    """`VoxelRaymarcher ... --trace OX,OY,OZ,DX,DY,DZ` (repeated) prints, after the frame is
    rendered and beside the pick lines, the line the Python trace gives for each ray."""
    xyz, rgb = golden_voxels()
    scene_path = str(tmp_path / "scene.vox")
    vr.write_voxel_file(scene_path, xyz, rgb)
    W, H, scale = 96, 64, 12
    rays = [(6.0, 2.0, 6.0, -6.0, -2.0, -7.0), (6.0, 2.0, 6.0, 0.0, 1.0, 0.0), (2.5, 3.0, 2.0, 0.0, -1.0, 0.25),
            (2.6, 2.7, 2.8, 0.0, 0.0, 0.0), (-4.0, 1.5, 2.5, 250.0, 10.0, 0.5), (6.0, 2.0, 6.0, -6.0, -2.0, -7.0)]
    out = str(tmp_path / "output.png")
    args = [EXE, str(scale), store, algo, "--scene", scene_path, "--width", str(W), "--height", str(H), "--out", out,
            "--pick", "48,32"]
    for r in rays:
        args += ["--trace", ",".join(repr(v) for v in r)]
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    got = [ln for ln in lines if ln.startswith("trace ")]
    with vr.create_scene(xyz, rgb, vr.parse_storage(store)) as scene:
        recs = vr.trace(scene, vr.parse_algorithm(algo), vr.VoxelSceneInfo(ZERO, scale), np.array(rays, np.float32))
    assert got == [trace_line(i, rec) for i, rec in enumerate(recs)]
    assert any(" voxel " in ln and " point " in ln for ln in got) and got[0][8:] == got[5][8:]
    # after the render and the picks, before the image is written
    order = [i for i, ln in enumerate(lines) if ln.startswith(("Execution Time", "pick ", "trace ", "Wrote "))]
    assert [lines[i].split()[0] for i in order] == ["Execution", "pick"] + ["trace"] * len(rays) + ["Wrote"]
    assert os.path.exists(out)


def test_cli_trace_refused_with_several_gpus(tmp_path):
    r = subprocess.run([EXE, "1", "vcs", "original", "--synth", "64", "--width", "64", "--height", "64", "--out",
                        str(tmp_path / "o.png"), "--gpus", "2", "--trace", "1,1,1,0,0,1"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "--trace" in r.stderr, r.stdout + r.stderr
    assert not os.path.exists(tmp_path / "o.png")
    for bad in ("1,2,3,4,5", "1,2,3;4,5,6", "1,2,3,4,5,6,7", "a,b,c,d,e,f"):
        r = subprocess.run([EXE, "1", "vcs", "original", "--trace", bad], capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--trace needs OX,OY,OZ,DX,DY,DZ" in r.stderr, bad
