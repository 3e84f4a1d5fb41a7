"""vr_shade on the GPU: the colour a render writes for a pixel, for any ray.

shade(camera_rays(frame)) is the render, word for word -- a second kernel with another lane
layout reproduces every pixel of gpu_render and of the oracle; for rays that are no pixel of a
camera the colours are held to the CPU reference (tests/shade_ref.py, tied to the oracle by
tests/test_shade_ref.py) and the optional records to vr_trace's bytes and tests/trace_ref.py:
both stores, both algorithms, every execution order, directional and point lights, shadows on
and off, several regions with a translation and a scale, bounce rays that start on voxel faces,
walks that crawl and walks that never end.  A shade is not a render launch and refuses what
vr_trace refuses."""
from __future__ import annotations

import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle
from tests import crawl_views, fuzz_cases, pick_ref, pyref, shade_ref, trace_cases, trace_ref
from tests.helpers import GOLDEN, diff_report, gpu_render, oracle_camera_from, oracle_lighting_from, render_learned

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


@functools.lru_cache(maxsize=None)
def golden_voxels():
    d = np.load(os.path.join(GOLDEN, "c1_scene.npz"))
    return d["xyz"], d["rgb"]


def frame_pixels(W, H):
    i = np.arange(W * H)
    return (i % W).astype(np.uint32), (i // W).astype(np.uint32)


def gpu_lighting(spec):
    """The library's lighting block of a shade_ref.LIGHTINGS entry (the same floats as
    shade_ref.pyref_lighting and, through oracle_lighting_from, as the oracle's)."""
    return shade_ref.fill_block(vr.setup_constant_values(), *spec)


@pytest.fixture(scope="module")
def golden_scenes():
    """The golden scene per store on the GPU, in the oracle and in pyref, built once."""
    xyz, rgb = golden_voxels()
    made = {s: (vr.create_scene(xyz, rgb, s), oracle.Scene(xyz, rgb, int(s)), pyref.Scene(xyz, rgb, int(s)))
            for s in (VCS, HASH)}
    yield made
    for g, o, _ in made.values():
        g.close()
        o.close()


def as_words(colors):
    """Colours of either form as a uint32 numpy array."""
    if torch.is_tensor(colors):
        assert colors.is_cuda and colors.dtype == torch.int32 and colors.dim() == 1
        return colors.cpu().numpy().view(np.uint32)
    assert isinstance(colors, np.ndarray) and colors.dtype == np.uint32 and colors.ndim == 1
    return colors


def assert_colors(got, want, where):
    got = as_words(got)
    assert got.shape == want.shape, where
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"{where}: {bad.size} of {len(want)} colours differ; first at ray {int(bad[0])}: "
                           f"gpu 0x{int(got[bad[0]]):06X} reference 0x{int(want[bad[0]]):06X}")


def assert_records(got, want, where):
    bad = pick_ref.same_records(got, want)
    assert bad.size == 0, (f"{where}: {bad.size} of {len(got)} records differ; first at ray {int(bad[0])}: "
                           f"gpu {got[bad[0]]} reference {want[bad[0]]}")


def shade_every_way(scene, algo, info, lit, rays, want, records, where):
    """Every order, hits NULL and hits given, host arrays and device tensors: the colours are
    `want` and the records have the bytes of `records` (vr_trace's or vr_pick's)."""
    drays = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()
    for order in ORDERS:
        tag = f"{where} {order.name}"
        assert_colors(vr.shade(scene, algo, info, lit, rays, order=order), want, tag)
        col, recs = scene.shade(algo, info, lit, rays, order=order, hits=True)
        assert_colors(col, want, tag + " with hits")
        assert recs.dtype == vr.HIT_DTYPE and recs.tobytes() == records.tobytes(), tag
        dcol = vr.shade(scene, algo, info, lit, drays, order=order)
        assert tuple(dcol.shape) == (len(rays),)
        assert_colors(dcol, want, tag + " on the device")
        dcol, drecs = vr.shade(scene, algo, info, lit, drays, order=order, hits=True)
        assert_colors(dcol, want, tag + " on the device with hits")
        assert drecs.is_cuda and drecs.dtype == torch.int32 and tuple(drecs.shape) == (len(rays), 16)
        assert drecs.cpu().numpy().tobytes() == records.tobytes(), tag


def lit_and_shadowed(on, off):
    """(pixels lit with shadows on, pixels 0 with shadows on and non-zero with shadows off)."""
    return int(np.count_nonzero(on)), int(np.count_nonzero((on == 0) & (off != 0)))


# ---------------------------------------------------------------- 1. the render, from rays

# floors on the oracle's 32 x 24 frames: (lit >=, shadowed >=).  Counted on the CPU for all four
# pairs: 343-347 / 219-221 (default light), 313-317 / 249-251 ((1, 2, 3)), 57-62 / 39-40 (point).
FRAME_FLOORS = {"directional": (300, 200), "directional-123": (300, 200), "point": (50, 30)}


@pytest.mark.parametrize("name", list(shade_ref.LIGHTINGS))
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_ID)
def test_shade_of_camera_rays_is_the_render(golden_scenes, pair, name):
    store, algo = pair
    scene, ref, _ = golden_scenes[store]
    spec = shade_ref.LIGHTINGS[name]
    W, H, scale = 32, 24, 12
    cam = vr.Camera.reference(W, H)
    info = vr.VoxelSceneInfo(ZERO, scale)
    lit = gpu_lighting(spec)
    px, py = frame_pixels(W, H)
    want, _ = ref.render(int(algo), oracle_camera_from(cam), oracle_lighting_from(lit), W, H, scale)
    frame, _ = gpu_render(scene, algo, cam, lit, info, W, H)
    assert np.array_equal(frame, want), "the render itself: " + diff_report(frame, want, W)
    if name in FRAME_FLOORS:       # the yardstick: an all-zero or an unshadowed kernel cannot pass
        off, _ = ref.render(int(algo), oracle_camera_from(cam), oracle_lighting_from(gpu_lighting(shade_ref.unshadowed(spec))),
                            W, H, scale)
        n_lit, n_shadowed = lit_and_shadowed(want, off)
        print(f"{PAIR_ID(pair)} {name}: lit {n_lit}, shadowed {n_shadowed}")
        assert n_lit >= FRAME_FLOORS[name][0] and n_shadowed >= FRAME_FLOORS[name][1], (n_lit, n_shadowed)
    else:
        assert np.count_nonzero(want) >= 500
    rays = vr.camera_rays(cam, W, H, px, py)
    shade_every_way(scene, algo, info, lit, rays, want, vr.pick(scene, algo, cam, info, W, H, px, py), name)
    if name == "directional-123":  # the other shadow arm: unequal components, and the library normalises alike
        assert not lit.light_dir[0] == lit.light_dir[1] == lit.light_dir[2]
        assert list(vr.setup_constant_values(light_direction=(1.0, 2.0, 3.0)).light_dir) == list(lit.light_dir)


# ---------------------------------------------------------------- 2. arbitrary rays

@functools.lru_cache(maxsize=None)
def golden_rays():
    """The 256 seeded rays of tests 2 and 6 (never modified)."""
    rays = trace_cases.random_rays(golden_voxels()[0], seed=11)
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def golden_reference(store, algo, name):
    """shade_ref's colours of golden_rays() at scale 1 with the lighting's shadows on and off,
    and which walks never end: computed once per (pair, lighting)."""
    xyz, rgb = golden_voxels()
    spec = shade_ref.LIGHTINGS[name]
    sc = pyref.Scene(xyz, rgb, int(store))
    on, never = shade_ref.shade_rays(sc, shade_ref.pyref_lighting(*spec), golden_rays(), 1, algo == LONGEST)
    off, _ = shade_ref.shade_rays(sc, shade_ref.pyref_lighting(*shade_ref.unshadowed(spec)), golden_rays(), 1, algo == LONGEST)
    for a in (on, off, never):
        a.setflags(write=False)
    return on, off, never


# floors on the reference's colours of the 256 rays: (lit >=, shadowed >=).  Counted on the CPU:
# directional 26-29 / 76-78 (VCS) and 29-31 / 75 (cuckoo, above the same floors: none is lowered);
# point light 14-19 / 37-39 (both stores).
RAY_FLOORS = {"directional": (20, 50), "point": (10, 30)}


@pytest.mark.parametrize("name", list(RAY_FLOORS))
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_ID)
def test_arbitrary_rays_match_reference(golden_scenes, pair, name):
    store, algo = pair
    scene = golden_scenes[store][0]
    rays = golden_rays()
    on, off, never = golden_reference(store, algo, name)
    n_lit, n_shadowed = lit_and_shadowed(on, off)
    print(f"{PAIR_ID(pair)} {name}: lit {n_lit}, shadowed {n_shadowed}, never {int(never.sum())}")
    assert n_lit >= RAY_FLOORS[name][0] and n_shadowed >= RAY_FLOORS[name][1], (n_lit, n_shadowed)
    info = vr.VoxelSceneInfo(ZERO, 1)
    lit = gpu_lighting(shade_ref.LIGHTINGS[name])
    records = vr.trace(scene, algo, info, rays, order=vr.TraceOrder.GIVEN)
    assert_records(records, trace_ref.trace_rays(golden_scenes[store][2], rays, 1, algo == LONGEST)[0], "vr_trace")
    shade_every_way(scene, algo, info, lit, rays, on, records, name)
    # shadows off: the other colours, the same records
    col, recs = vr.shade(scene, algo, info, gpu_lighting(shade_ref.unshadowed(shade_ref.LIGHTINGS[name])), rays, hits=True)
    assert_colors(col, off, name + " unshadowed")
    assert recs.tobytes() == records.tobytes()
    # the (n, 6) form and the empty call
    flat = np.concatenate([rays["origin"], rays["direction"]], axis=1)
    assert_colors(vr.shade(scene, algo, info, lit, flat), on, "(n, 6)")
    empty = vr.shade(scene, algo, info, lit, np.zeros(0, vr.RAY_DTYPE), hits=True)
    assert len(empty[0]) == 0 and len(empty[1]) == 0


# ---------------------------------------------------------------- 3. several regions

@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_ID)
def test_several_regions_negative_coordinates_translated_scaled(pair):
    """tests/fuzz_cases.py make_wide_case(81): voxels from (-122, -248, -192) to (77, -49, 6) over
    several 64^3 regions, scale 2, translation (-3.5, 4.5, -6.5); a point light at the centre of
    the voxels' box, in the lighting's world space (translation + voxel coordinates)."""
    store, algo = pair
    c = fuzz_cases.make_wide_case(81)
    assert c.scale == 2 and c.translation == (-3.5, 4.5, -6.5) and c.xyz.min() < -64 and np.ptp(c.xyz, axis=0).min() > 128
    lo, hi = c.xyz.min(axis=0), c.xyz.max(axis=0)
    pos = tuple(float(t + (a + b + 1) / 2.0) for t, a, b in zip(c.translation, lo, hi))
    assert pos == (-25.5, -143.5, -99.0)
    spec = (True, True, pos, None)
    rays = trace_cases.random_rays(c.xyz, seed=12, scale=c.scale, translation=c.translation)
    sc = pyref.Scene(c.xyz, c.rgb, int(store))
    on, _ = shade_ref.shade_rays(sc, shade_ref.pyref_lighting(*spec), rays, c.scale, algo == LONGEST, c.translation)
    off, _ = shade_ref.shade_rays(sc, shade_ref.pyref_lighting(*shade_ref.unshadowed(spec)), rays, c.scale, algo == LONGEST,
                                  c.translation)
    # (the light's attenuation over these distances leaves few colours above 0: 8 lit and 8
    # shadowed for every pair, counted on the CPU; the floors only keep the case from going blank)
    n_lit, n_shadowed = lit_and_shadowed(on, off)
    print(f"{PAIR_ID(pair)}: lit {n_lit}, shadowed {n_shadowed}")
    assert n_lit >= 5 and n_shadowed >= 5, (n_lit, n_shadowed)
    want_recs, _ = trace_ref.trace_rays(sc, rays, c.scale, algo == LONGEST, c.translation)
    info = vr.VoxelSceneInfo(c.translation, c.scale)
    with vr.create_scene(c.xyz, c.rgb, store) as scene:
        records = vr.trace(scene, algo, info, rays)
        assert_records(records, want_recs, "vr_trace")
        shade_every_way(scene, algo, info, gpu_lighting(spec), rays, on, records, "wide")
        assert_colors(vr.shade(scene, algo, info, gpu_lighting(shade_ref.unshadowed(spec)), rays), off, "wide unshadowed")
    hit = records[records["status"] == vr.HitStatus.VOXEL]
    assert (hit["voxel"] < 0).any() and (hit["region"] < 0).any() and len(np.unique(hit["region"], axis=0)) > 1


# ---------------------------------------------------------------- 4. bounce rays

@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_ID)
def test_bounce_rays_from_picked_points(golden_scenes, pair):
    """One mirror bounce of the golden frame: from the world position of each VOXEL record's
    `point` (on a voxel face) along the pixel's direction mirrored in the record's normal."""
    store, algo = pair
    scene, _, sc = golden_scenes[store]
    W, H, scale = 32, 24, 12
    cam = vr.Camera.reference(W, H)
    info = vr.VoxelSceneInfo(ZERO, scale)
    px, py = frame_pixels(W, H)
    first = vr.pick(scene, algo, cam, info, W, H, px, py)
    primary = vr.camera_rays(cam, W, H, px, py)
    keep = first["status"] == vr.HitStatus.VOXEL
    assert np.count_nonzero(keep) >= 500
    rec, d = first[keep], primary["direction"][keep].astype(np.float32)
    n = rec["normal"].astype(np.float32)
    # world = translation + (region * 64 + point) / scale, in float32 (translation 0)
    origin = ((rec["region"] * 64).astype(np.float32) + rec["point"]) / np.float32(scale)
    mirrored = d - np.float32(2.0) * np.sum(d * n, axis=1, keepdims=True, dtype=np.float32) * n
    rays = trace_ref.rays_of(origin, mirrored)
    lit_spec = shade_ref.LIGHTINGS["directional"]
    want, _ = shade_ref.shade_rays(sc, shade_ref.pyref_lighting(*lit_spec), rays, scale, algo == LONGEST)
    want_recs, _ = trace_ref.trace_rays(sc, rays, scale, algo == LONGEST)
    # the bounce sees something: second hits, some of them lit
    assert np.count_nonzero(want_recs["status"] == trace_ref.VOXEL) >= 20 and np.count_nonzero(want) >= 5
    for order in ORDERS:
        col, recs = vr.shade(scene, algo, info, gpu_lighting(lit_spec), rays, order=order, hits=True)
        assert_colors(col, want, f"bounce {order.name}")
        assert_records(recs, want_recs, f"bounce {order.name}")
    assert_colors(vr.shade(scene, algo, info, gpu_lighting(lit_spec), rays), want, "bounce, no hits")


# ---------------------------------------------------------------- 5. crawls

@pytest.mark.parametrize("algo", [ORIGINAL, LONGEST], ids=lambda a: a.name)
@pytest.mark.parametrize("view", [v for v in crawl_views.VIEWS if v.name in ("x-plane-from-behind", "shadow-x-point-light")],
                         ids=lambda v: v.name)
def test_crawling_walks_are_fast_forwarded(view, algo):
    """A view whose primary walks crawl and one whose shadow walks do (tests/crawl_views.py: walks
    of 65 536 to ~10^6 iterations, tests/test_gpu_crawl_views.py holds the views to that): the
    camera rays of the whole 48 x 32 frame, every pixel the crawl-view test renders, against
    oracle.Scene.render_pixels.  (In the oracle x-plane-from-behind has 48 such primary walks --
    each ends in a miss, as in every primary view -- beside 53 lit pixels; the shadow view has 11
    to 14 such shadow walks, 8 to 11 of them behind a lit pixel, among 715 to 736 lit pixels.)"""
    W, H = crawl_views.W, crawl_views.H
    xyz, rgb = crawl_views.SCENES[view.scene]()
    cam = vr.Camera(view.world(view.eye), view.world(view.look_at), crawl_views.UP, view.fov, crawl_views.ASPECT)
    lit = vr.setup_constant_values(use_point_light=view.point, light_position=view.light_pos,
                                   light_direction=view.light_dir)
    info = vr.VoxelSceneInfo(view.translation, view.scale)
    px, py = frame_pixels(W, H)
    ref = oracle.Scene(xyz, rgb, oracle.STORE_VCS)
    want, _ = ref.render_pixels(int(algo), oracle_camera_from(cam), oracle_lighting_from(lit), W, H, view.scale, px, py,
                                view.translation)
    ref.close()
    assert np.count_nonzero(want) >= 20
    rays = vr.camera_rays(cam, W, H, px, py)
    with vr.create_scene(xyz, rgb, VCS) as scene:
        assert_colors(vr.shade(scene, algo, info, lit, rays), want, view.name)
        col, recs = vr.shade(scene, algo, info, lit, rays, hits=True)
        assert_colors(col, want, view.name + " with hits")
        assert recs.tobytes() == vr.pick(scene, algo, cam, info, W, H, px, py).tobytes()


# ---------------------------------------------------------------- 6. walks that never end

def test_walks_that_never_end_give_zero(golden_scenes):
    """A zero direction normalises to NaN: from inside the scene the original walk never
    finishes -- colour 0, status NEVER.  And whatever shade_ref reports as never ending among
    the arbitrary rays is 0 on the GPU."""
    info = vr.VoxelSceneInfo(ZERO, 1)
    lit = gpu_lighting(shade_ref.LIGHTINGS["directional"])
    ray = trace_ref.rays_of([(30.5, 40.25, 20.75)], [(0.0, 0.0, 0.0)])
    for store in (VCS, HASH):
        scene, _, sc = golden_scenes[store]
        assert shade_ref.shade_walk(sc, shade_ref.pyref_lighting(*shade_ref.LIGHTINGS["directional"]), ray[0]["origin"],
                                    ray[0]["direction"], 1, False) == (0, True)
        for order in ORDERS:
            col, recs = vr.shade(scene, ORIGINAL, info, lit, ray, order=order, hits=True)
            assert int(col[0]) == 0 and int(recs[0]["status"]) == vr.HitStatus.NEVER
            assert recs[0].tobytes()[4:] == bytes(60)
            assert int(vr.shade(scene, ORIGINAL, info, lit, ray, order=order)[0]) == 0
    for store, algo in PAIRS:
        for name in RAY_FLOORS:
            on, _, never = golden_reference(store, algo, name)
            got = vr.shade(golden_scenes[store][0], algo, info, gpu_lighting(shade_ref.LIGHTINGS[name]), golden_rays())
            assert not got[never].any() and not on[never].any()


# ---------------------------------------------------------------- 7. not a render

def test_shade_is_not_a_render_launch(golden_scenes):
    """The vr_debug_order_uses counters do not move over shades, and a view that has learned its
    orders renders the same frame after them, still under those orders."""
    scene, ref, _ = golden_scenes[VCS]
    W, H, scale = 64, 48, 12
    cam = vr.Camera.reference(W, H)
    info = vr.VoxelSceneInfo(ZERO, scale)
    lit = vr.setup_constant_values()
    px, py = frame_pixels(W, H)
    rays = vr.camera_rays(cam, W, H, px, py)
    want, _ = ref.render(int(ORIGINAL), oracle_camera_from(cam), oracle_lighting_from(lit), W, H, scale)
    vr.forget_orders(0)
    bad, first, d = render_learned(scene, ORIGINAL, cam, lit, info, W, H, 0, H, want, None, 0)
    assert not bad, diff_report(first, want, W)
    assert d["lane_order_uses"] >= d["slots"] + 1 and d["work_order_uses"] >= d["slots"] + 1, d
    uses = vr.debug_order_uses(0)
    for order in ORDERS:
        assert_colors(vr.shade(scene, ORIGINAL, info, lit, rays, order=order), want, order.name)
        assert_colors(vr.shade(scene, ORIGINAL, info, lit, rays, order=order, hits=True)[0], want, order.name)
    assert vr.debug_order_uses(0) == uses      # (not a render launch: no counter moves)
    bad, first, d = render_learned(scene, ORIGINAL, cam, lit, info, W, H, 0, H, want, None, 0, launches=3)
    assert not bad, diff_report(first, want, W)
    assert d["lane_order_uses"] == 3 and d["work_order_uses"] == 3 and d["lane_orders_made"] == 0 and \
        d["work_orders_made"] == 0, d


# ---------------------------------------------------------------- 8. refusals on the device

def raw_shade(scene, algo, info, lit, rays, n, colors, hits, in_dev, out_dev, order):
    """vr_shade itself, on the caller's buffers (numpy arrays, CUDA tensors or plain addresses)."""
    def ptr(a):
        if a is None:
            return None
        return ctypes.c_void_p(a if isinstance(a, int) else (a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data))
    vr._capi.check(vr.lib().vr_shade(scene.handle, int(algo), ctypes.byref(lit), vr._capi.f3(info.translation),
                                     int(info.scale), ptr(rays), n, int(in_dev), ptr(colors), ptr(hits), int(out_dev),
                                     int(order), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "vr_shade")


def test_bad_device_buffers_and_orders_are_refused(golden_scenes):
    scene = golden_scenes[VCS][0]
    info = vr.VoxelSceneInfo(ZERO, 1)
    lit = gpu_lighting(shade_ref.LIGHTINGS["directional"])
    n = 64
    drays = torch.from_numpy(golden_rays().view(np.float32).reshape(-1, 8).copy()).cuda()
    dh = torch.full((n + 1, 16), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    dc = torch.full((n + 1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    cases = [(drays.data_ptr() + 4, dc, dh, vr.TraceOrder.GIVEN, "aligned"),
             (drays, dc, dh.data_ptr() + 8, vr.TraceOrder.GIVEN, "aligned"),
             (drays, dc.data_ptr() + 2, dh, vr.TraceOrder.GIVEN, "aligned"),
             (drays, dc.data_ptr() + 1, None, vr.TraceOrder.COHERENT, "aligned"),
             (drays, dc, dh, 3, "order"), (drays, dc, None, 0xFFFFFFFF, "order")]
    for rays, colors, hits, order, word in cases:
        with pytest.raises(vr.VrError) as e:
            raw_shade(scene, ORIGINAL, info, lit, rays, n, colors, hits, True, True, order)
        assert e.value.code == -1 and "vr_shade" in str(e.value) and word in str(e.value)
    # host buffers with an unknown order: untouched too
    hc, hh = np.full(n, 0xABABABAB, np.uint32), np.full(n, 0xAB, np.uint8).repeat(64).view(vr.HIT_DTYPE)
    with pytest.raises(vr.VrError):
        raw_shade(scene, ORIGINAL, info, lit, golden_rays(), n, hc, hh, False, False, 5)
    torch.cuda.synchronize()
    assert (dh == 0x5A5A5A5A).all() and (dc == 0x5A5A5A5A).all()
    assert (hc == 0xABABABAB).all() and hh.tobytes() == bytes([0xAB]) * 64 * n
    # the same buffers, well formed: n words and n records, the sentinels beyond them kept
    raw_shade(scene, ORIGINAL, info, lit, drays, n, dc, dh, True, True, vr.TraceOrder.COHERENT)
    on, _, _ = golden_reference(VCS, ORIGINAL, "directional")
    assert_colors(dc[:n], on[:n], "device buffers")
    assert int(dc[n]) == 0x5A5A5A5A and (dh[n] == 0x5A5A5A5A).all()
    assert dh[:n].cpu().numpy().tobytes() == vr.trace(scene, ORIGINAL, info, golden_rays()[:n]).tobytes()


# ---------------------------------------------------------------- 9. the CLI

def g9(x):
    """printf's %.9g (which, unlike Python's format, prints a NaN's sign: "-nan")."""
    x = float(x)
    return ("-nan" if np.signbit(x) else "nan") if np.isnan(x) else f"{x:.9g}"


def shade_line(i, color, r):
    head = f"shade {i} color 0x{int(color):06X} "
    if int(r["status"]) == vr.HitStatus.VOXEL:
        v, n, p = r["voxel"], r["normal"], r["point"]
        return head + (f"voxel {v[0]} {v[1]} {v[2]} color 0x{int(r['color']):06X} normal {n[0]} {n[1]} {n[2]} "
                       f"point {g9(p[0])} {g9(p[1])} {g9(p[2])}")
    return head + {0: "miss", 2: "never"}[int(r["status"])]


@pytest.mark.parametrize("store,algo,flags", [("vcs", "original", []), ("hashtable", "longestaxis", ["--no-shadows"])])
def test_cli_shade(tmp_path, store, algo, flags):
    """`VoxelRaymarcher ... --shade OX,OY,OZ,DX,DY,DZ` (repeated) prints, after the trace lines,
    `shade <i> color 0x%06X` and the --trace text of the ray's record: the Python call's values
    for the run's scale and lighting flags."""
    xyz, rgb = golden_voxels()
    scene_path = str(tmp_path / "scene.vox")
    vr.write_voxel_file(scene_path, xyz, rgb)
    W, H, scale = 96, 64, 12
    rays = [(6.0, 2.0, 6.0, -6.0, -2.0, -7.0), (6.0, 2.0, 6.0, 0.0, 1.0, 0.0), (2.5, 3.0, 2.0, 0.0, -1.0, 0.25)]
    out = str(tmp_path / "output.png")
    args = [EXE, str(scale), store, algo, "--scene", scene_path, "--width", str(W), "--height", str(H), "--out", out,
            "--trace", "6,2,6,-6,-2,-7"] + flags
    for r in rays:
        args += ["--shade", ",".join(repr(v) for v in r)]
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    got = [ln for ln in lines if ln.startswith("shade ")]
    lit = vr.setup_constant_values(use_shadows=not flags)
    with vr.create_scene(xyz, rgb, vr.parse_storage(store)) as scene:
        col, recs = vr.shade(scene, vr.parse_algorithm(algo), vr.VoxelSceneInfo(ZERO, scale), lit,
                             np.array(rays, np.float32), hits=True)
    assert got == [shade_line(i, c, rec) for i, (c, rec) in enumerate(zip(col, recs))]
    assert " voxel " in got[0] and " point " in got[0] and got[1] == "shade 1 color 0x000000 miss"
    order = [i for i, ln in enumerate(lines) if ln.startswith(("Execution Time", "trace ", "shade ", "Wrote "))]
    assert [lines[i].split()[0] for i in order] == ["Execution", "trace"] + ["shade"] * len(rays) + ["Wrote"]
    # single-GPU only, and a malformed ray is refused, as for --trace
    r = subprocess.run([EXE, "1", "vcs", "original", "--synth", "64", "--width", "64", "--height", "64", "--out",
                        str(tmp_path / "o.png"), "--gpus", "2", "--shade", "1,1,1,0,0,1"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "--shade" in r.stderr, r.stdout + r.stderr
    r = subprocess.run([EXE, "1", "vcs", "original", "--shade", "1,2,3,4,5"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--shade needs OX,OY,OZ,DX,DY,DZ" in r.stderr
