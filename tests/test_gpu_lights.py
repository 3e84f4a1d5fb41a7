"""vr_shade_lights on the GPU: several of the reference's lights and an ambient term for any rays,
from one primary walk per ray.

The words are held to the CPU reference (tests/lights_ref.py, tied to the C oracle by
tests/test_lights_ref.py) on the golden frame under four lights and an ambient term, for both
stores and both algorithms, every execution order, with and without records, from host arrays and
device tensors; one light is vr_shade; no light is the ambient term alone; the order of the
lights changes nothing; arbitrary rays, several regions with a translation and a scale, shadow
walks that crawl and a walk that never ends; the call is not a render launch and refuses what
vr_shade refuses; render_lights and the CLI's --add-light / --ambient frame are the same words."""
from __future__ import annotations

import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle
from tests import crawl_views, fuzz_cases, lights_cases, lights_ref, pyref, shade_ref, trace_cases, trace_ref
from tests.helpers import diff_report, oracle_camera_from, oracle_lighting_from, render_learned
from tests.test_png import decode_png

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
W, H, SCALE = lights_cases.W, lights_cases.H, lights_cases.SCALE


def gpu_light(light):
    """The library's lighting block of a lights_ref light (the same floats as lights_ref.pyref_light)."""
    return lights_ref.fill_block(vr.setup_constant_values(), light)


def frame_pixels(w, h):
    i = np.arange(w * h)
    return (i % w).astype(np.uint32), (i // w).astype(np.uint32)


@pytest.fixture(scope="module")
def golden_scenes():
    """The golden scene per store on the GPU, built once."""
    xyz, rgb = lights_cases.golden_voxels()
    made = {s: vr.create_scene(xyz, rgb, s) for s in (VCS, HASH)}
    yield made
    for g in made.values():
        g.close()


@functools.lru_cache(maxsize=None)
def frame_rays():
    """The frame's camera rays as the library makes them: the bytes of the reference's."""
    rays = vr.camera_rays(vr.Camera.reference(W, H), W, H, *frame_pixels(W, H))
    assert rays.tobytes() == lights_cases.frame_rays().tobytes()
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def frame_want(store, algo, ambient=True):
    """lights_ref's words of the golden frame under the four lights, with or without the ambient term."""
    terms, amb = lights_cases.frame_terms(int(store), algo == LONGEST)
    want = lights_ref.combine(list(terms) + ([amb] if ambient else []))
    want.setflags(write=False)
    return want


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


def shade_lights_every_way(scene, algo, info, lights, ambient, rays, want, records, where):
    """Every order, hits NULL and hits given, host arrays and device tensors: the colours are
    `want` and the records have the bytes of `records` (vr_trace's or vr_pick's)."""
    drays = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()
    for order in ORDERS:
        tag = f"{where} {order.name}"
        assert_colors(vr.shade_lights(scene, algo, info, lights, rays, ambient=ambient, order=order), want, tag)
        col, recs = scene.shade_lights(algo, info, lights, rays, ambient=ambient, order=order, hits=True)
        assert_colors(col, want, tag + " with hits")
        assert recs.dtype == vr.HIT_DTYPE and recs.tobytes() == records.tobytes(), tag
        dcol = vr.shade_lights(scene, algo, info, lights, drays, ambient=ambient, order=order)
        assert tuple(dcol.shape) == (len(rays),)
        assert_colors(dcol, want, tag + " on the device")
        dcol, drecs = vr.shade_lights(scene, algo, info, lights, drays, ambient=ambient, order=order, hits=True)
        assert_colors(dcol, want, tag + " on the device with hits")
        assert drecs.is_cuda and drecs.dtype == torch.int32 and tuple(drecs.shape) == (len(rays), 16)
        assert drecs.cpu().numpy().tobytes() == records.tobytes(), tag


# ---------------------------------------------------------------- 1. four lights and an ambient term

@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_ID)
def test_golden_frame_four_lights_and_ambient(golden_scenes, pair):
    store, algo = pair
    scene = golden_scenes[store]
    info = vr.VoxelSceneInfo(ZERO, SCALE)
    want = frame_want(store, algo)
    # (the case is not vacuous: tests/test_lights_ref.py holds its floors; here, counted on the CPU
    # for every pair, 593-595 words are non-zero and the ambient term changes 579-581 of them)
    assert np.count_nonzero(want) >= 500 and np.count_nonzero(want != frame_want(store, algo, ambient=False)) >= 500
    lights = [gpu_light(l) for l in lights_ref.LIGHTS]
    records = vr.pick(scene, algo, vr.Camera.reference(W, H), info, W, H, *frame_pixels(W, H))
    shade_lights_every_way(scene, algo, info, lights, lights_ref.AMBIENT, frame_rays(), want, records, PAIR_ID(pair))
    # without the ambient term, and the (n, 6) form
    assert_colors(vr.shade_lights(scene, algo, info, lights, frame_rays()), frame_want(store, algo, ambient=False), "no ambient")
    flat = np.concatenate([frame_rays()["origin"], frame_rays()["direction"]], axis=1)
    assert_colors(vr.shade_lights(scene, algo, info, lights, flat, ambient=lights_ref.AMBIENT), want, "(n, 6)")
    empty = vr.shade_lights(scene, algo, info, lights, np.zeros(0, vr.RAY_DTYPE), hits=True)
    assert len(empty[0]) == 0 and len(empty[1]) == 0


# ---------------------------------------------------------------- 2. one light, no light

@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_ID)
def test_one_light_is_vr_shade_and_no_light_is_the_ambient_term(golden_scenes, pair):
    store, algo = pair
    scene = golden_scenes[store]
    info = vr.VoxelSceneInfo(ZERO, SCALE)
    rays = frame_rays()
    records = vr.trace(scene, algo, info, rays)
    for name, spec in shade_ref.LIGHTINGS.items():
        lit = shade_ref.fill_block(vr.setup_constant_values(), *spec)
        one = vr.shade(scene, algo, info, lit, rays)
        assert not (one >> 24).any() and np.count_nonzero(one) >= 50, name
        col, recs = vr.shade_lights(scene, algo, info, [lit], rays, hits=True)
        assert_colors(col, one, name)
        assert recs.tobytes() == records.tobytes(), name
    # a coloured, shadowed light too (lights_ref's B), against the reference's term
    terms, amb = lights_cases.frame_terms(int(store), algo == LONGEST)
    assert_colors(vr.shade_lights(scene, algo, info, [gpu_light(lights_ref.LIGHT_B)], rays), terms[1], "light B")
    # no light: the ambient term alone, at every primary hit and nowhere else
    hit = records["status"] == vr.HitStatus.VOXEL
    assert np.count_nonzero(hit) >= 500 and np.count_nonzero(~hit) >= 100
    want_amb = lights_ref.sat_add_rgb(0, amb)
    assert np.count_nonzero(want_amb) >= 500 and not want_amb[~hit].any()
    for order in ORDERS:
        col, recs = vr.shade_lights(scene, algo, info, [], rays, ambient=lights_ref.AMBIENT, order=order, hits=True)
        assert_colors(col, want_amb, f"ambient alone {order.name}")
        assert recs.tobytes() == records.tobytes()
    # an ambient term above 1: channels past 255 bleed in the term's packing, bits 24-31 are dropped
    big = (3.0, 1.0, 2.0)
    sc = lights_cases.pyref_scene(int(store))
    want_big = lights_ref.sat_add_rgb(0, lights_ref.ambient_terms(sc, big, rays, SCALE, algo == LONGEST))
    assert_colors(vr.shade_lights(scene, algo, info, [], rays, ambient=big), want_big, "ambient above 1")
    # neither: all zeros, the records intact
    col, recs = vr.shade_lights(scene, algo, info, [], rays, hits=True)
    assert not col.any() and recs.tobytes() == records.tobytes()
    dcol = vr.shade_lights(scene, algo, info, [], torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda())
    assert not as_words(dcol).any()


# ---------------------------------------------------------------- 3. the order of the lights

@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_ID)
def test_light_order_changes_nothing(golden_scenes, pair):
    store, algo = pair
    scene = golden_scenes[store]
    info = vr.VoxelSceneInfo(ZERO, SCALE)
    lights = [gpu_light(l) for l in lights_ref.LIGHTS]
    want = frame_want(store, algo)
    for order in ([3, 2, 1, 0], [2, 0, 3, 1]):
        got = vr.shade_lights(scene, algo, info, [lights[k] for k in order], frame_rays(), ambient=lights_ref.AMBIENT)
        assert_colors(got, want, f"lights in order {order}")
    # the same light many times over saturates: VR_MAX_LIGHTS copies of D are min(255, 64 * channel)
    terms, _ = lights_cases.frame_terms(int(store), algo == LONGEST)
    d = terms[3]
    sums = np.stack([(d >> 16) & 0xFF, (d >> 8) & 0xFF, d & 0xFF], axis=1).astype(np.int64) * 64
    packed = np.minimum(sums, 255).astype(np.uint32)
    got = vr.shade_lights(scene, algo, info, [lights[3]] * 64, frame_rays())
    assert_colors(got, packed[:, 0] << 16 | packed[:, 1] << 8 | packed[:, 2], "64 lights")
    with pytest.raises(vr.VrError) as e:
        vr.shade_lights(scene, algo, info, [lights[3]] * 65, frame_rays())
    assert e.value.code == -1 and "VR_MAX_LIGHTS" in str(e.value)


# ---------------------------------------------------------------- 4. arbitrary rays

@functools.lru_cache(maxsize=None)
def golden_rays():
    """The first 203 (no multiple of 64 or 256) of the 256 seeded rays of tests/test_gpu_shade.py."""
    rays = trace_cases.random_rays(lights_cases.golden_voxels()[0], seed=11)[:203].copy()
    rays.setflags(write=False)
    return rays


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_ID)
def test_arbitrary_rays_match_reference(golden_scenes, pair):
    store, algo = pair
    scene = golden_scenes[store]
    rays = golden_rays()
    three = (lights_ref.LIGHT_A, lights_ref.LIGHT_B, lights_ref.LIGHT_C)
    sc = lights_cases.pyref_scene(int(store))
    terms = lights_ref.light_terms(sc, three, rays, 1, algo == LONGEST)
    amb = lights_ref.ambient_terms(sc, lights_ref.AMBIENT, rays, 1, algo == LONGEST)
    lit = [int(np.count_nonzero(t)) for t in terms]
    print(f"{PAIR_ID(pair)}: lit per light {lit}, ambient {int(np.count_nonzero(amb))}")
    # (counted on the CPU with tests/pyref.py for all four pairs: 17-21 rays lit under A, 22-23 under
    # B, 8-12 under C, 165-168 with an ambient term; the floors only keep the case from going blank)
    assert lit[0] >= 15 and lit[2] >= 5 and np.count_nonzero(amb) >= 60, lit
    info = vr.VoxelSceneInfo(ZERO, 1)
    records = vr.trace(scene, algo, info, rays, order=vr.TraceOrder.GIVEN)
    shade_lights_every_way(scene, algo, info, [gpu_light(l) for l in three], lights_ref.AMBIENT, rays,
                           lights_ref.combine(terms + [amb]), records, "arbitrary")
    assert_colors(vr.shade_lights(scene, algo, info, [gpu_light(l) for l in three], rays), lights_ref.combine(terms),
                  "arbitrary, no ambient")


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_ID)
def test_several_regions_negative_coordinates_translated_scaled(pair):
    """tests/fuzz_cases.py make_wide_case(81), as tests/test_gpu_shade.py takes it: several regions,
    negative coordinates, scale 2, translation (-3.5, 4.5, -6.5); a point light at the centre of the
    voxels' box and the directional light B."""
    store, algo = pair
    c = fuzz_cases.make_wide_case(81)
    assert c.scale == 2 and c.translation == (-3.5, 4.5, -6.5) and c.xyz.min() < -64 and np.ptp(c.xyz, axis=0).min() > 128
    two = ((True, True, (-25.5, -143.5, -99.0), None, (1.0, 1.0, 1.0)), lights_ref.LIGHT_B)
    rays = trace_cases.random_rays(c.xyz, seed=12, scale=c.scale, translation=c.translation)
    sc = pyref.Scene(c.xyz, c.rgb, int(store))
    terms = lights_ref.light_terms(sc, two, rays, c.scale, algo == LONGEST, c.translation)
    amb = lights_ref.ambient_terms(sc, lights_ref.AMBIENT, rays, c.scale, algo == LONGEST, c.translation)
    lit = [int(np.count_nonzero(t)) for t in terms]
    print(f"{PAIR_ID(pair)}: lit per light {lit}, ambient {int(np.count_nonzero(amb))}")
    # (counted on the CPU for every pair: 8 rays lit by the point light, 10 by B, 30 with an ambient term)
    assert lit[0] >= 5 and lit[1] >= 5 and np.count_nonzero(amb) >= 20, lit
    info = vr.VoxelSceneInfo(c.translation, c.scale)
    with vr.create_scene(c.xyz, c.rgb, store) as scene:
        records = vr.trace(scene, algo, info, rays)
        shade_lights_every_way(scene, algo, info, [gpu_light(l) for l in two], lights_ref.AMBIENT, rays,
                               lights_ref.combine(terms + [amb]), records, "wide")
    hit = records[records["status"] == vr.HitStatus.VOXEL]
    assert (hit["voxel"] < 0).any() and (hit["region"] < 0).any() and len(np.unique(hit["region"], axis=0)) > 1


# ---------------------------------------------------------------- 5. crawls and walks that never end

@pytest.mark.parametrize("algo", [ORIGINAL, LONGEST], ids=lambda a: a.name)
def test_shadow_walks_that_crawl_under_one_of_two_lights(algo):
    """tests/crawl_views.py "shadow-x": shadow walks of 65 536 to ~10^6 iterations towards the
    light (-0.004, 0.7, 0.7), beside the default light, whose shadow walks do not crawl: the whole
    48 x 32 frame against the oracle's two frames, combined."""
    view = next(v for v in crawl_views.VIEWS if v.name == "shadow-x")
    w, h = crawl_views.W, crawl_views.H
    xyz, rgb = crawl_views.SCENES[view.scene]()
    cam = vr.Camera(view.world(view.eye), view.world(view.look_at), crawl_views.UP, view.fov, crawl_views.ASPECT)
    lights = [vr.setup_constant_values(light_direction=view.light_dir), vr.setup_constant_values()]
    info = vr.VoxelSceneInfo(view.translation, view.scale)
    px, py = frame_pixels(w, h)
    ref = oracle.Scene(xyz, rgb, oracle.STORE_VCS)
    frames = [ref.render_pixels(int(algo), oracle_camera_from(cam), oracle_lighting_from(l), w, h, view.scale, px, py,
                                view.translation)[0] for l in lights]
    ref.close()
    assert all(np.count_nonzero(f) >= 20 for f in frames) and np.count_nonzero(frames[0] != frames[1]) >= 20
    want = lights_ref.combine(frames)
    rays = vr.camera_rays(cam, w, h, px, py)
    with vr.create_scene(xyz, rgb, VCS) as scene:
        assert_colors(vr.shade_lights(scene, algo, info, lights, rays), want, view.name)
        col, recs = vr.shade_lights(scene, algo, info, lights[::-1], rays, hits=True)
        assert_colors(col, want, view.name + " reversed, with hits")
        assert recs.tobytes() == vr.pick(scene, algo, cam, info, w, h, px, py).tobytes()


def test_a_walk_that_never_ends_gives_zero_even_with_ambient(golden_scenes):
    """A zero direction normalises to NaN: from inside the scene the original walk never finishes
    -- colour 0 and status NEVER, whatever the lights and the ambient term."""
    info = vr.VoxelSceneInfo(ZERO, 1)
    lights = [gpu_light(l) for l in lights_ref.LIGHTS]
    ray = trace_ref.rays_of([(30.5, 40.25, 20.75)], [(0.0, 0.0, 0.0)])
    for store in (VCS, HASH):
        scene = golden_scenes[store]
        for order in ORDERS:
            col, recs = vr.shade_lights(scene, ORIGINAL, info, lights, ray, ambient=(1.0, 1.0, 1.0), order=order, hits=True)
            assert int(col[0]) == 0 and int(recs[0]["status"]) == vr.HitStatus.NEVER
            assert recs[0].tobytes()[4:] == bytes(60)
            assert int(vr.shade_lights(scene, ORIGINAL, info, lights, ray, ambient=(1.0, 1.0, 1.0), order=order)[0]) == 0
            assert int(vr.shade_lights(scene, ORIGINAL, info, [], ray, ambient=(1.0, 1.0, 1.0), order=order)[0]) == 0


# ---------------------------------------------------------------- 6. not a render; refusals on the device

def test_shade_lights_is_not_a_render_launch(golden_scenes):
    """The vr_debug_order_uses counters do not move over the calls, and a view that has learned its
    orders renders the same frame after them, still under those orders."""
    scene = golden_scenes[VCS]
    xyz, rgb = lights_cases.golden_voxels()
    w, h = 64, 48
    cam = vr.Camera.reference(w, h)
    info = vr.VoxelSceneInfo(ZERO, SCALE)
    lit = vr.setup_constant_values()
    ref = oracle.Scene(xyz, rgb, oracle.STORE_VCS)
    want, _ = ref.render(int(ORIGINAL), oracle_camera_from(cam), oracle_lighting_from(lit), w, h, SCALE)
    ref.close()
    rays = vr.camera_rays(cam, w, h, *frame_pixels(w, h))
    vr.forget_orders(0)
    bad, first, d = render_learned(scene, ORIGINAL, cam, lit, info, w, h, 0, h, want, None, 0)
    assert not bad, diff_report(first, want, w)
    uses = vr.debug_order_uses(0)
    for order in ORDERS:
        assert_colors(vr.shade_lights(scene, ORIGINAL, info, [lit], rays, order=order), want, order.name)
        vr.shade_lights(scene, ORIGINAL, info, [lit, gpu_light(lights_ref.LIGHT_D)], rays, ambient=lights_ref.AMBIENT,
                        order=order, hits=True)
    assert vr.debug_order_uses(0) == uses      # (not a render launch: no counter moves)
    bad, first, d = render_learned(scene, ORIGINAL, cam, lit, info, w, h, 0, h, want, None, 0, launches=3)
    assert not bad, diff_report(first, want, w)
    assert d["lane_order_uses"] == 3 and d["work_order_uses"] == 3 and d["lane_orders_made"] == 0 and \
        d["work_orders_made"] == 0, d


def raw_shade_lights(scene, algo, info, lights, ambient, rays, n, colors, hits, in_dev, out_dev, order):
    """vr_shade_lights itself, on the caller's buffers (numpy arrays, CUDA tensors or plain addresses)."""
    def ptr(a):
        if a is None:
            return None
        return ctypes.c_void_p(a if isinstance(a, int) else (a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data))
    block = (vr._capi.VrLighting * len(lights))(*lights)
    vr._capi.check(vr.lib().vr_shade_lights(scene.handle, int(algo), block, len(lights), vr._capi.f3(ambient),
                                            vr._capi.f3(info.translation), int(info.scale), ptr(rays), n, int(in_dev),
                                            ptr(colors), ptr(hits), int(out_dev), int(order),
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "vr_shade_lights")


def test_bad_device_buffers_are_refused_and_sentinels_kept(golden_scenes):
    scene = golden_scenes[VCS]
    info = vr.VoxelSceneInfo(ZERO, 1)
    lights = [gpu_light(l) for l in (lights_ref.LIGHT_A, lights_ref.LIGHT_B, lights_ref.LIGHT_C)]
    n = 67                 # (one full wave and three lanes of the next)
    rays = golden_rays()
    drays = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()
    dh = torch.full((n + 1, 16), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    dc = torch.full((n + 1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    cases = [(drays.data_ptr() + 4, dc, dh, vr.TraceOrder.GIVEN, "aligned"),
             (drays, dc, dh.data_ptr() + 8, vr.TraceOrder.GIVEN, "aligned"),
             (drays, dc.data_ptr() + 2, dh, vr.TraceOrder.GIVEN, "aligned"),
             (drays, dc.data_ptr() + 1, None, vr.TraceOrder.COHERENT, "aligned"),
             (drays, dc, dh, 3, "order"), (drays, dc, None, 0xFFFFFFFF, "order")]
    for r, colors, hits, order, word in cases:
        with pytest.raises(vr.VrError) as e:
            raw_shade_lights(scene, ORIGINAL, info, lights, lights_ref.AMBIENT, r, n, colors, hits, True, True, order)
        assert e.value.code == -1 and "vr_shade_lights" in str(e.value) and word in str(e.value)
    # host buffers with an unknown order: untouched too
    hc, hh = np.full(n, 0xABABABAB, np.uint32), np.full(n, 0xAB, np.uint8).repeat(64).view(vr.HIT_DTYPE)
    with pytest.raises(vr.VrError):
        raw_shade_lights(scene, ORIGINAL, info, lights, lights_ref.AMBIENT, rays, n, hc, hh, False, False, 5)
    torch.cuda.synchronize()
    assert (dh == 0x5A5A5A5A).all() and (dc == 0x5A5A5A5A).all()
    assert (hc == 0xABABABAB).all() and hh.tobytes() == bytes([0xAB]) * 64 * n
    # the same buffers, well formed: n words and n records, the sentinels beyond them kept
    sc = lights_cases.pyref_scene(int(VCS))
    want = lights_ref.shade_lights_rays(sc, (lights_ref.LIGHT_A, lights_ref.LIGHT_B, lights_ref.LIGHT_C), rays[:n], 1, False,
                                        ambient=lights_ref.AMBIENT)
    for order in (vr.TraceOrder.COHERENT, vr.TraceOrder.GIVEN):
        dc.fill_(0x5A5A5A5A)
        dh.fill_(0x5A5A5A5A)
        raw_shade_lights(scene, ORIGINAL, info, lights, lights_ref.AMBIENT, drays, n, dc, dh, True, True, order)
        assert_colors(dc[:n], want, f"device buffers {order.name}")
        assert int(dc[n]) == 0x5A5A5A5A and (dh[n] == 0x5A5A5A5A).all()
        assert dh[:n].cpu().numpy().tobytes() == vr.trace(scene, ORIGINAL, info, rays[:n]).tobytes()


# ---------------------------------------------------------------- 7. render_lights and the CLI

@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_ID)
def test_render_lights_is_the_frame(golden_scenes, pair):
    store, algo = pair
    scene = golden_scenes[store]
    info = vr.VoxelSceneInfo(ZERO, SCALE)
    lights = [gpu_light(l) for l in lights_ref.LIGHTS]
    frame = vr.render_lights(scene, algo, vr.Camera.reference(W, H), info, lights, W, H, ambient=lights_ref.AMBIENT)
    assert frame.is_cuda and frame.dtype == torch.int32 and tuple(frame.shape) == (H, W)
    assert_colors(frame.reshape(-1), frame_want(store, algo), "render_lights")
    # a frame whose sides are no multiples of 8: every pixel written once, the words of its rays
    w, h = 29, 19
    cam = vr.Camera.reference(w, h)
    frame = vr.render_lights(scene, algo, cam, info, lights[:2], w, h)
    want = vr.shade_lights(scene, algo, info, lights[:2], vr.camera_rays(cam, w, h, *frame_pixels(w, h)))
    assert np.count_nonzero(want) >= 100
    assert_colors(frame.reshape(-1), want, "render_lights 29 x 19")


@pytest.mark.parametrize("store,algo,flags", [("vcs", "original", []), ("hashtable", "longestaxis", ["--no-shadows"])])
def test_cli_lights_frame(tmp_path, store, algo, flags):
    """`VoxelRaymarcher ... --add-light DX,DY,DZ,R,G,B --add-light ... --ambient R,G,B` writes the
    vr_shade_lights frame -- the run's own light, then the added ones -- and says so in one line."""
    xyz, rgb = lights_cases.golden_voxels()
    scene_path = str(tmp_path / "scene.vox")
    vr.write_voxel_file(scene_path, xyz, rgb)
    w, h, scale = 93, 61, 12
    out = str(tmp_path / "output.png")
    added = [((-2.0, 1.0, 3.0), (0.5, 0.75, 1.0)), ((1.0, 2.0, 3.0), (1.0, 0.5, 0.25))]
    args = [EXE, str(scale), store, algo, "--scene", scene_path, "--width", str(w), "--height", str(h), "--out", out] + flags
    for d, c in added:
        args += ["--add-light", ",".join(repr(v) for v in d + c)]
    args += ["--ambient", "0.25,0.125,0.0625"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert "lights 3 ambient 0.25 0.125 0.0625" in lines
    assert lines.index("lights 3 ambient 0.25 0.125 0.0625") < next(i for i, ln in enumerate(lines) if ln.startswith("Wrote "))
    lights = [vr.setup_constant_values(use_shadows=not flags)]
    lights += [vr.setup_constant_values(use_shadows=not flags, light_direction=d, light_color=c) for d, c in added]
    with vr.create_scene(xyz, rgb, vr.parse_storage(store)) as scene:
        frame = vr.render_lights(scene, vr.parse_algorithm(algo), vr.Camera.reference(w, h), vr.VoxelSceneInfo(ZERO, scale),
                                 lights, w, h, ambient=(0.25, 0.125, 0.0625))
    words = frame.cpu().numpy().view(np.uint32)
    assert np.count_nonzero(words) >= 1000
    want = np.stack([(words >> 16) & 0xFF, (words >> 8) & 0xFF, words & 0xFF], axis=2).astype(np.uint8)
    got = decode_png(open(out, "rb").read())
    assert got.shape == (h, w, 3) and np.array_equal(got, want)


def test_cli_lights_refusals(tmp_path):
    base = [EXE, "1", "vcs", "original", "--synth", "64", "--width", "64", "--height", "64", "--out", str(tmp_path / "o.png")]
    for extra in (["--add-light", "1,1,1,1,1,1"], ["--ambient", "0.5,0.5,0.5"]):
        r = subprocess.run(base + ["--gpus", "2"] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--add-light" in r.stderr and "--gpus" in r.stderr, r.stdout + r.stderr
    r = subprocess.run(base + ["--add-light", "1,2,3,4,5"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--add-light needs DX,DY,DZ,R,G,B" in r.stderr
    r = subprocess.run(base + ["--ambient", "1,2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--ambient needs R,G,B" in r.stderr
    r = subprocess.run(base + ["--add-light"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--add-light needs a value" in r.stderr
