"""vr_bounce_rays and vr_shade_lights_reflect on the GPU, word for word against tests/reflect_ref.py,
for both stores and both algorithms:

 (a) the golden frame (tests/reflect_cases.py): bounces 1..4, reflectivity 255 and 96, occlusion off,
     AMBIENT at 96 and ALL at 255, with and without hits and return_ao, every order, host arrays
     and device tensors; render_lights(reflect=...), also with samples=2; the CLI's --reflect frame;
 (b) reflect=0 or bounces=0 is shade_lights(ao=...);
 (c) the call equals the fold, in torch integer ops, of shade_lights over bounce_rays of its own
     hits and rays, depth by depth; bounce_rays' bytes on the golden and on made-up records;
 (d) mirror tests: a material bit, a painted key colour, a mask that matches nothing, all-miss rays;
 (e) a corridor between two mirror slabs, where every ray hits at every depth;
 (f) tests/lattice_cases.py' scene and lattice rays in every form (scale 3 with a translation,
     negative regions);
 (g) odd sizes with guard words; (h) refusals on the device; (i) nothing learned or forgotten.

Every test here needs the new entry points."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle
from tests import ao_cases, ao_ref, lattice_cases, lights_cases, lights_ref, reflect_cases, reflect_ref
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
# occlusion settings: (shade_lights' keywords, reflect_ref's strength and apply)
AOS = [({}, None, ao_ref.AMBIENT), (dict(ao=96, ao_apply=vr.AoApply.AMBIENT), 96, ao_ref.AMBIENT),
       (dict(ao=255, ao_apply=vr.AoApply.ALL), 255, ao_ref.ALL)]
ZERO = (0.0, 0.0, 0.0)
W, H, SCALE = reflect_cases.W, reflect_cases.H, reflect_cases.SCALE
GUARD = 0x5A5A5A5A


@pytest.fixture(scope="module")
def golden_scenes():
    xyz, rgb = lights_cases.golden_voxels()
    made = {s: vr.create_scene(xyz, rgb, s) for s in (VCS, HASH)}
    yield made
    for g in made.values():
        g.close()


def gpu_lights(lights=lights_ref.LIGHTS):
    return [lights_ref.fill_block(vr.setup_constant_values(), l) for l in lights]


def words(a):
    """Words of either form as a uint32 numpy array."""
    if torch.is_tensor(a):
        assert a.is_cuda and a.dtype == torch.int32 and a.dim() == 1
        return a.cpu().numpy().view(np.uint32)
    assert isinstance(a, np.ndarray) and a.dtype == np.uint32 and a.ndim == 1
    return a


def assert_words(got, want, where):
    got = words(got)
    assert got.shape == want.shape, where
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"{where}: {bad.size} of {len(want)} words differ; first at {int(bad[0])}: "
                           f"gpu 0x{int(got[bad[0]]):06X} reference 0x{int(want[bad[0]]):06X}")


def device_rays(rays):
    return torch.from_numpy(np.ascontiguousarray(rays).view(np.float32).reshape(-1, 8).copy()).cuda()


def device_records(recs):
    return torch.from_numpy(np.ascontiguousarray(recs).view(np.int32).reshape(-1, 16).copy()).cuda()


# ---------------------------------------------------------------- (a) the golden frame

@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_ID)
def test_golden_frame(golden_scenes, pair):
    store, algo = pair
    scene = golden_scenes[store]
    longest = algo == LONGEST
    info = vr.VoxelSceneInfo(ZERO, SCALE)
    rays = lights_cases.frame_rays()
    drays = device_rays(rays)
    lights = gpu_lights()
    amb = lights_ref.AMBIENT
    records = ao_cases.frame_records(int(store), longest)
    want_ao = ao_cases.frame_ao(int(store), longest)
    assert vr.trace(scene, algo, info, rays).tobytes() == records.tobytes()
    turn = 0
    for bounces in (1, 2, 3, 4):
        for k in (255, 96):
            for kw_ao, strength, apply in AOS:
                want = reflect_cases.golden_words(int(store), longest, k, bounces, strength=strength, apply=apply)
                shallower = reflect_cases.golden_words(int(store), longest, k, bounces - 1, strength=strength, apply=apply)
                assert np.count_nonzero(want != shallower) >= 5        # (this depth shows)
                # every order at the first and the last depth, one in turn at the others
                for order in (ORDERS if bounces in (1, 4) else [ORDERS[turn % 3]]):
                    turn += 1
                    tag = f"{PAIR_ID(pair)} bounces={bounces} k={k} ao={strength} {order.name}"
                    kw = dict(ambient=amb, order=order, reflect=k, bounces=bounces, **kw_ao)
                    assert_words(vr.shade_lights(scene, algo, info, lights, rays, **kw), want, tag)
                    col, recs = scene.shade_lights(algo, info, lights, rays, hits=True, **kw)
                    assert_words(col, want, tag + " with hits")
                    assert recs.tobytes() == records.tobytes(), tag
                    assert_words(vr.shade_lights(scene, algo, info, lights, drays, **kw), want, tag + " on the device")
                    dcol, drecs = vr.shade_lights(scene, algo, info, lights, drays, hits=True, **kw)
                    assert_words(dcol, want, tag + " on the device with hits")
                    assert drecs.cpu().numpy().tobytes() == records.tobytes(), tag
                    if strength is None:
                        continue
                    col, ao = vr.shade_lights(scene, algo, info, lights, rays, return_ao=True, **kw)
                    assert_words(col, want, tag + " with ao")
                    assert_words(ao, want_ao, tag + " ao")
                    dcol, drecs, dao = vr.shade_lights(scene, algo, info, lights, drays, hits=True, return_ao=True, **kw)
                    assert_words(dcol, want, tag + " on the device with hits and ao")
                    assert_words(dao, want_ao, tag + " ao on the device")
                    assert drecs.cpu().numpy().tobytes() == records.tobytes(), tag
                    assert_words(dao, words(vr.occlusion(scene, drecs)), tag + " vr_occlusion's values")
    # no light and no ambient term: black at every depth; no light: the ambient terms alone
    assert not words(vr.shade_lights(scene, algo, info, [], rays, reflect=200, bounces=2)).any()
    lv = reflect_cases.golden_levels(int(store), longest)
    bare = [reflect_ref.Level(l.idx, l.rays, l.recs, [], l.amb, l.ao, l.refl) for l in lv]
    assert_words(vr.shade_lights(scene, algo, info, [], rays, ambient=amb, reflect=200, bounces=3),
                 reflect_ref.fold(bare, 200, 3), "no light")


@pytest.mark.parametrize("pair", [PAIRS[0], PAIRS[3]], ids=PAIR_ID)
def test_render_lights_with_reflect(golden_scenes, pair):
    store, algo = pair
    scene = golden_scenes[store]
    longest = algo == LONGEST
    info = vr.VoxelSceneInfo(ZERO, SCALE)
    cam = vr.Camera.reference(W, H)
    for kw_ao, strength, apply in AOS[:2]:
        frame = vr.render_lights(scene, algo, cam, info, gpu_lights(), W, H, ambient=lights_ref.AMBIENT, reflect=96, bounces=2,
                                 **kw_ao)
        assert frame.is_cuda and frame.dtype == torch.int32 and tuple(frame.shape) == (H, W)
        assert_words(frame.reshape(-1), reflect_cases.golden_words(int(store), longest, 96, 2, strength=strength, apply=apply),
                     f"render_lights ao={strength}")
    frame = vr.render_lights(scene, algo, cam, info, gpu_lights(), W, H, ambient=lights_ref.AMBIENT, reflect=255, bounces=4,
                             mirror=reflect_cases.BIT)
    assert_words(frame.reshape(-1), reflect_cases.golden_words(int(store), longest, 255, 4, reflect_cases.BIT), "render_lights, bit")
    # samples=: the arguments pass through to the fine frame unchanged; the fine frame at 2 W x 2 H
    # holds the golden frame's rays at no pixel, so it is held to the plain call and the filter
    w, h = 13, 9
    args = (scene, algo, vr.Camera.reference(2 * w, 2 * h), info, gpu_lights(), 2 * w, 2 * h)
    fine = vr.render_lights(*args, ambient=lights_ref.AMBIENT, reflect=128, bounces=2, mirror=reflect_cases.BIT)
    plain = vr.render_lights(*args, ambient=lights_ref.AMBIENT)
    assert int((fine != plain).sum()) >= 10
    got = vr.render_lights(scene, algo, vr.Camera.reference(w, h), info, gpu_lights(), w, h, ambient=lights_ref.AMBIENT,
                           reflect=128, bounces=2, mirror=reflect_cases.BIT, samples=2)
    assert torch.equal(got, vr.resolve(fine, w, h, 2))


@pytest.mark.parametrize("store,algo", [("vcs", "original"), ("hashtable", "longestaxis")])
def test_cli_reflect_frame(tmp_path, store, algo):
    """`VoxelRaymarcher ... --reflect K [--bounces B] [--mirror RRGGBB]` writes the
    vr_shade_lights_reflect frame and ends its "lights" line in "reflect <K> bounces <B> mirror <...>"."""
    xyz, rgb = lights_cases.golden_voxels()
    _, painted, _ = reflect_cases.painted_voxels()      # every third voxel in the key colour
    key = reflect_cases.KEY
    scene_path, painted_path = str(tmp_path / "scene.vox"), str(tmp_path / "painted.vox")
    vr.write_voxel_file(scene_path, xyz, rgb)
    vr.write_voxel_file(painted_path, xyz, np.array(painted))
    out = str(tmp_path / "output.png")
    base = [EXE, str(SCALE), store, algo, "--scene", scene_path, "--width", str(W), "--height", str(H), "--out", out]
    longest = algo == "longestaxis"
    st = int(vr.parse_storage(store))

    def png_words():
        px = decode_png(open(out, "rb").read()).astype(np.uint32)
        return (px[..., 0] << 16 | px[..., 1] << 8 | px[..., 2]).reshape(-1)

    # the run's own light, an ambient term, occlusion: the golden frame under lights_ref.LIGHT_A
    r = subprocess.run(base + ["--ambient", "0.25,0.25,0.25", "--ao", "96", "--reflect", "96", "--bounces", "3"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "lights 1 ambient 0.25 0.25 0.25 ao 96 ambient reflect 96 bounces 3 mirror every" in r.stdout.splitlines()
    lv = reflect_cases.golden_levels(st, longest)
    one = [reflect_ref.Level(l.idx, l.rays, l.recs, l.terms[:1], l.amb, l.ao, l.refl) for l in lv]
    assert lights_ref.LIGHTS[0] == lights_ref.LIGHT_A
    assert_words(png_words(), reflect_ref.fold(one, 96, 3, 96, ao_ref.AMBIENT), "--reflect 96 --bounces 3")
    # --reflect alone selects the lights frame, one bounce; --mirror a key colour under mask 0xFFFFFF
    keyed_base = [painted_path if a == scene_path else a for a in base]
    r = subprocess.run(keyed_base + ["--reflect", "255", "--mirror", "%06x" % key], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"lights 1 ambient 0 0 0 reflect 255 bounces 1 mirror {key:06x}" in r.stdout.splitlines()
    with vr.create_scene(xyz, np.array(painted), vr.parse_storage(store)) as scene:
        args = (scene, vr.parse_algorithm(algo), vr.Camera.reference(W, H), vr.VoxelSceneInfo(ZERO, SCALE), [vr.setup_constant_values()],
                W, H)
        keyed = vr.render_lights(*args, reflect=255, mirror=(0xFFFFFF, key))
        plain = vr.render_lights(*args)
    with vr.create_scene(xyz, rgb, vr.parse_storage(store)) as scene:
        # --aa: the fine frame, resolved
        fine = vr.render_lights(scene, vr.parse_algorithm(algo), vr.Camera.reference(W, H), vr.VoxelSceneInfo(ZERO, SCALE),
                                [vr.setup_constant_values()], W, H, reflect=200, bounces=2, samples=2)
    assert int((keyed != plain).sum()) >= 10
    assert_words(png_words(), words(keyed.reshape(-1)), "--mirror")
    r = subprocess.run(base + ["--reflect", "200", "--bounces", "2", "--aa", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert_words(png_words(), words(fine.reshape(-1)), "--reflect with --aa")
    # refusals need no device work
    for extra, word in ((["--reflect", "256"], "--reflect needs K"), (["--reflect", "x"], "--reflect needs K"),
                        (["--reflect", "9", "--bounces", "5"], "--bounces needs B"), (["--bounces", "2"], "need --reflect"),
                        (["--mirror", "ff00ff"], "need --reflect"), (["--reflect", "9", "--mirror", "1234567"], "--mirror needs RRGGBB"),
                        (["--reflect", "9", "--mirror", "zz"], "--mirror needs RRGGBB"), (["--reflect", "5", "--gpus", "2"], "--gpus")):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and word in r.stderr, r.stdout + r.stderr


# ---------------------------------------------------------------- (b) the null case

@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_ID)
def test_no_reflectivity_or_no_depth_is_shade_lights(golden_scenes, pair):
    store, algo = pair
    scene = golden_scenes[store]
    info = vr.VoxelSceneInfo(ZERO, SCALE)
    rays = lights_cases.frame_rays()
    lights = gpu_lights()
    for kw_ao, strength, apply in AOS:
        plain, recs = vr.shade_lights(scene, algo, info, lights, rays, ambient=lights_ref.AMBIENT, hits=True, **kw_ao)
        assert_words(plain, ao_cases.frame_words(int(store), algo == LONGEST, strength, apply), f"the plain call, ao={strength}")
        for k, bounces in ((0, 1), (0, 4), (255, 0), (96, 0), (0, 0)):
            for mirror in (None, reflect_cases.BIT):
                tag = f"reflect={k} bounces={bounces} mirror={mirror} ao={strength}"
                kw = dict(ambient=lights_ref.AMBIENT, reflect=k, bounces=bounces, mirror=mirror, **kw_ao)
                assert_words(vr.shade_lights(scene, algo, info, lights, rays, **kw), words(plain), tag)
                c2, r2 = vr.shade_lights(scene, algo, info, lights, device_rays(rays), hits=True, **kw)
                assert_words(c2, words(plain), tag + " on the device")
                assert r2.cpu().numpy().tobytes() == recs.tobytes()
    for bad, word in ((dict(reflect=256), "reflectivity"), (dict(reflect=1, bounces=5), "VR_MAX_BOUNCES"),
                      (dict(reflect=1, mirror=(1, 3)), "mirror_value")):
        with pytest.raises(vr.VrError) as e:
            vr.shade_lights(scene, algo, info, lights, rays, **bad)
        assert e.value.code == -1 and "vr_shade_lights_reflect" in str(e.value) and word in str(e.value)
    with pytest.raises(ValueError):
        vr.shade_lights(scene, algo, info, lights, rays, bounces=2)
    with pytest.raises(ValueError):
        vr.shade_lights(scene, algo, info, lights, rays, mirror=(1, 1))


# ---------------------------------------------------------------- (c) composition on the device

def torch_mix(a, b, k):
    a, b = a.long() & 0xFFFFFFFF, b.long() & 0xFFFFFFFF
    out = torch.zeros_like(a)
    for sh in (16, 8, 0):
        out |= ((((a >> sh) & 0xFF) * (255 - k) + ((b >> sh) & 0xFF) * k + 127) // 255) << sh
    return out.int()


def composed(scene, algo, info, lights, drays, k, bounces, mirror, **kw):
    """The call's words from the public calls it stands for: shade_lights per depth over bounce_rays
    of the depth above, masked by what is alive (a ray that is not has an all-NaN bounce, whose
    word is not used), folded from the back in torch integer ops."""
    cols, refls = [], []
    alive = torch.ones(drays.shape[0], dtype=torch.bool, device=drays.device)
    cur = drays
    for j in range(bounces + 1):
        c, h = vr.shade_lights(scene, algo, info, lights, cur, hits=True, **kw)
        cols.append(torch.where(alive, c, torch.zeros_like(c)))
        alive = alive & (h[:, 0] == 1) & ((h[:, 1] & mirror[0]) == mirror[1])
        refls.append(alive)
        if j < bounces:
            cur = vr.bounce_rays(cur, h, info)
    out = cols[bounces]
    for j in range(bounces - 1, -1, -1):
        out = torch.where(refls[j], torch_mix(cols[j], out, k), cols[j])
    return out, [int(r.sum()) for r in refls]


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_ID)
def test_the_call_is_the_fold_of_its_public_parts(golden_scenes, pair):
    store, algo = pair
    scene = golden_scenes[store]
    info = vr.VoxelSceneInfo(ZERO, SCALE)
    drays = device_rays(lights_cases.frame_rays())
    lights = gpu_lights()
    for k, bounces, mirror, kw_ao in ((128, 3, (0, 0), AOS[0][0]), (255, 4, (1, 1), AOS[1][0]), (37, 2, (0, 0), AOS[2][0])):
        kw = dict(ambient=lights_ref.AMBIENT, **kw_ao)
        want, counts = composed(scene, algo, info, lights, drays, k, bounces, mirror, **kw)
        assert counts == reflect_ref.alive_counts(reflect_cases.golden_levels(int(store), algo == LONGEST, mirror))[: bounces + 1]
        got = vr.shade_lights(scene, algo, info, lights, drays, reflect=k, bounces=bounces, mirror=mirror, **kw)
        assert_words(got, words(want), f"{PAIR_ID(pair)} k={k} bounces={bounces} mirror={mirror}")


def raw_bounce_rays(info, rays, hits, n, out, in_dev, out_dev):
    def ptr(a):
        return ctypes.c_void_p(a if isinstance(a, int) else (a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data))
    vr._capi.check(vr.lib().vr_bounce_rays(0, vr._capi.f3(info.translation), int(info.scale), ptr(rays), ptr(hits), n, int(in_dev),
                                           ptr(out), int(out_dev), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
                   "vr_bounce_rays")


def test_bounce_rays_bytes():
    rays = lights_cases.frame_rays()
    cases = [(rays, ao_cases.frame_records(st, lg), SCALE, ZERO) for st, lg in reflect_cases.PAIRS]
    cases += [(rays, ao_cases.frame_records(1, True), 3, lattice_cases.TRANSLATION)]
    cases += [reflect_cases.made_up() + form for form in reflect_cases.MADE_UP_FORMS]
    for rr, recs, scale, tr in cases:
        info = vr.VoxelSceneInfo(tr, scale)
        want = reflect_ref.bounce(rr, recs, scale, tr)
        got = vr.bounce_rays(rr, recs, info)
        assert got.dtype == vr.RAY_DTYPE and got.tobytes() == want.tobytes(), (scale, tr)
        dgot = vr.bounce_rays(device_rays(rr), device_records(recs), info)
        assert dgot.is_cuda and dgot.dtype == torch.float32 and tuple(dgot.shape) == (len(rr), 8)
        assert dgot.cpu().numpy().tobytes() == want.tobytes(), (scale, tr)
        # (n, 6) rays on both sides
        six = np.concatenate([rr["origin"], rr["direction"]], axis=1)
        assert vr.bounce_rays(six, recs, info).tobytes() == want.tobytes()
        assert vr.bounce_rays(torch.from_numpy(six).cuda(), device_records(recs), info).cpu().numpy().tobytes() == want.tobytes()
    assert len(vr.bounce_rays(np.zeros(0, vr.RAY_DTYPE), np.zeros(0, vr.HIT_DTYPE), vr.VoxelSceneInfo(ZERO, 1))) == 0
    # odd sizes, with a guard ray after the output, in every staging
    rr, recs = reflect_cases.made_up()
    scale, tr = reflect_cases.MADE_UP_FORMS[2]
    info = vr.VoxelSceneInfo(tr, scale)
    want = reflect_ref.bounce(rr, recs, scale, tr).view(np.uint32).reshape(-1, 8)
    dr, dh = device_rays(rr), device_records(recs)
    for n in (1, 63, 64, 65, 257):
        dout = torch.full((n + 1, 8), GUARD, dtype=torch.int32, device="cuda")
        raw_bounce_rays(info, dr, dh, n, dout, True, True)
        assert np.array_equal(dout[:n].cpu().numpy().view(np.uint32), want[:n]) and bool((dout[n] == GUARD).all()), n
        hout = np.full((n + 1, 8), GUARD, dtype=np.uint32)
        raw_bounce_rays(info, np.ascontiguousarray(rr), np.ascontiguousarray(recs), n, hout, False, False)
        assert np.array_equal(hout[:n], want[:n]) and (hout[n] == GUARD).all(), n
        dout.fill_(GUARD)
        raw_bounce_rays(info, np.ascontiguousarray(rr), np.ascontiguousarray(recs), n, dout, False, True)
        assert np.array_equal(dout[:n].cpu().numpy().view(np.uint32), want[:n]) and bool((dout[n] == GUARD).all()), n
    with pytest.raises(TypeError):
        vr.bounce_rays(dr, recs, info)
    with pytest.raises(ValueError):
        vr.bounce_rays(rr[:5], recs[:4], info)


# ---------------------------------------------------------------- (d) mirror selection

@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_ID)
def test_material_bit(golden_scenes, pair):
    store, algo = pair
    scene = golden_scenes[store]
    longest = algo == LONGEST
    info = vr.VoxelSceneInfo(ZERO, SCALE)
    rays = lights_cases.frame_rays()
    lights = gpu_lights()
    every = reflect_cases.golden_words(int(store), longest, 255, 4)
    for bounces, k, (kw_ao, strength, apply) in ((1, 255, AOS[0]), (2, 96, AOS[1]), (3, 255, AOS[2]), (4, 96, AOS[0]), (4, 255, AOS[1])):
        want = reflect_cases.golden_words(int(store), longest, k, bounces, reflect_cases.BIT, strength=strength, apply=apply)
        got = vr.shade_lights(scene, algo, info, lights, rays, ambient=lights_ref.AMBIENT, reflect=k, bounces=bounces,
                              mirror=reflect_cases.BIT, **kw_ao)
        assert_words(got, want, f"mirror=(1, 1) bounces={bounces} k={k} ao={strength}")
    assert np.count_nonzero(every != reflect_cases.golden_words(int(store), longest, 255, 4, reflect_cases.BIT)) >= 100
    # a mask that matches nothing: the plain call (no ray is left at depth 1)
    stored = set(lights_cases.golden_voxels()[1].tolist())
    absent = next(c for c in range(1, 1 << 24) if c not in stored)
    plain = ao_cases.frame_words(int(store), longest, None)
    for order in ORDERS:
        col, recs = vr.shade_lights(scene, algo, info, lights, rays, ambient=lights_ref.AMBIENT, reflect=255, bounces=4,
                                    mirror=(0xFFFFFF, absent), order=order, hits=True)
        assert_words(col, plain, f"a mirror test that nothing passes, {order.name}")
        assert recs.tobytes() == ao_cases.frame_records(int(store), longest).tobytes()
    # a frame of rays that all miss: from far outside the scene's frame, outwards
    away = np.array(rays)
    away["origin"] = (500.0, 400.0, 300.0)
    away["direction"] = np.abs(away["direction"]) + np.float32(0.01)
    col, recs = vr.shade_lights(scene, algo, info, lights, away, ambient=lights_ref.AMBIENT, reflect=255, bounces=4, hits=True)
    assert not words(col).any() and not recs["status"].any()
    assert not words(vr.shade_lights(scene, algo, info, lights, device_rays(away), ambient=lights_ref.AMBIENT, reflect=96, bounces=2,
                                     ao=255)).any()


@pytest.mark.parametrize("pair", [PAIRS[1], PAIRS[2]], ids=PAIR_ID)
def test_painted_key_colour(pair):
    store, algo = pair
    longest = algo == LONGEST
    xyz, rgb = lights_cases.golden_voxels()
    _, painted, which = reflect_cases.painted_voxels()
    lv = reflect_cases.painted_levels(int(store), longest)
    counts = reflect_ref.alive_counts(lv)
    assert counts[0] >= 100 and counts[1] >= 20 and counts[0] < len(lv[0].idx) - 100     # some rays reflect, some do not
    info = vr.VoxelSceneInfo(ZERO, SCALE)
    rays = lights_cases.frame_rays()
    with vr.create_scene(xyz, rgb, store) as scene:
        assert scene.paint(xyz[which], np.full(len(which), reflect_cases.KEY, dtype=np.uint32)) == 0
        for k, bounces, (kw_ao, strength, apply) in ((255, 1, AOS[0]), (96, 2, AOS[1]), (255, 2, AOS[2])):
            got = vr.shade_lights(scene, algo, info, gpu_lights(), rays, ambient=lights_ref.AMBIENT, reflect=k, bounces=bounces,
                                  mirror=reflect_cases.KEY_MIRROR, **kw_ao)
            assert_words(got, reflect_ref.fold(lv, k, bounces, strength, apply), f"painted mirrors k={k} bounces={bounces}")


# ---------------------------------------------------------------- (e) the mirror corridor

@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_ID)
def test_mirror_corridor(pair):
    store, algo = pair
    lv = reflect_cases.corridor_levels(int(store), algo == LONGEST)
    assert reflect_ref.alive_counts(lv) == [reflect_cases.CORRIDOR_N] * 5          # every ray hits at every depth
    xyz, rgb = reflect_cases.corridor_voxels()
    rays = reflect_cases.corridor_rays()
    info = vr.VoxelSceneInfo(ZERO, 1)
    with vr.create_scene(xyz, rgb, store) as scene:
        for k in (128, 255):
            for kw_ao, strength, apply in AOS[:2]:
                got = vr.shade_lights(scene, algo, info, gpu_lights(reflect_cases.CORRIDOR_LIGHTS), rays,
                                      ambient=reflect_cases.CORRIDOR_AMBIENT, reflect=k, bounces=4, **kw_ao)
                assert_words(got, reflect_ref.fold(lv, k, 4, strength, apply), f"corridor k={k} ao={strength}")
        deep = reflect_ref.fold(lv, 255, 4)
        assert np.count_nonzero(deep) >= 250 and np.count_nonzero(deep != reflect_ref.fold(lv, 255, 3)) >= 100


# ---------------------------------------------------------------- (f) roundings and frames

@pytest.mark.parametrize("store", [VCS, HASH], ids=lambda s: s.name)
def test_lattice_rays_in_every_form(store):
    xyz, rgb = lattice_cases.scene_voxels()
    with vr.create_scene(xyz, rgb, store) as scene:
        for form, (scale, tr) in lattice_cases.FORMS.items():
            rays = lattice_cases.family_rays("lattice", form)
            info = vr.VoxelSceneInfo(tr, scale)
            for algo in (ORIGINAL, LONGEST):
                lv = reflect_cases.lattice_levels(form, int(store), algo == LONGEST)
                counts = reflect_ref.alive_counts(lv)
                assert len(lv) == 3 and counts[0] >= 150 and counts[1] >= 100, (form, counts)
                assert (lv[1].recs["region"] < 0).any()
                for k, (kw_ao, strength, apply) in ((255, AOS[0]), (96, AOS[2])):
                    got, recs = vr.shade_lights(scene, algo, info, gpu_lights(reflect_cases.LATTICE_LIGHTS), np.array(rays),
                                                ambient=lights_ref.AMBIENT, reflect=k, bounces=reflect_cases.LATTICE_BOUNCES,
                                                hits=True, **kw_ao)
                    assert_words(got, reflect_ref.fold(lv, k, 2, strength, apply), f"{form} {store.name} {algo.name} k={k}")
                    assert recs.tobytes() == lv[0].recs.tobytes()


# ---------------------------------------------------------------- (g) sizes

def raw_reflect(scene, algo, info, lights, ambient, rays, n, colors, hits, ao_out, in_dev, out_dev, strength, apply, k, bounces,
                mirror=(0, 0), order=0):
    def ptr(a):
        if a is None:
            return None
        return ctypes.c_void_p(a if isinstance(a, int) else (a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data))
    block = (vr._capi.VrLighting * len(lights))(*lights)
    vr._capi.check(vr.lib().vr_shade_lights_reflect(
        scene.handle, int(algo), block, len(lights), vr._capi.f3(ambient), vr._capi.f3(info.translation), int(info.scale), ptr(rays),
        n, int(in_dev), ptr(colors), ptr(hits), int(out_dev), int(order), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream),
        strength, apply, ptr(ao_out), k, bounces, mirror[0], mirror[1]), "vr_shade_lights_reflect")


@pytest.mark.parametrize("store", [VCS, HASH], ids=lambda s: s.name)
def test_odd_sizes_and_the_words_after_the_outputs(golden_scenes, store):
    scene = golden_scenes[store]
    info = vr.VoxelSceneInfo(ZERO, SCALE)
    start = 200
    rays = np.ascontiguousarray(lights_cases.frame_rays()[start:start + 257])
    drays = device_rays(rays)
    lights = gpu_lights()
    want = reflect_cases.golden_words(int(store), False, 96, 3, strength=96, apply=ao_ref.ALL)[start:start + 257]
    plain = ao_cases.frame_words(int(store), False, 96, ao_ref.ALL)[start:start + 257]
    want_ao = ao_cases.frame_ao(int(store), False)[start:start + 257]
    for n in (1, 63, 64, 65, 255, 256, 257):
        assert n == 1 or np.count_nonzero(want[:n] != plain[:n]) >= 1
        dc = torch.full((n + 1,), GUARD, dtype=torch.int32, device="cuda")
        da = torch.full((n + 1,), GUARD, dtype=torch.int32, device="cuda")
        raw_reflect(scene, ORIGINAL, info, lights, lights_ref.AMBIENT, drays, n, dc, None, da, True, True, 96, 1, 96, 3)
        assert_words(dc[:n], want[:n], f"n = {n} on the device")
        assert_words(da[:n], want_ao[:n], f"n = {n} ao on the device")
        assert int(dc[n]) == GUARD and int(da[n]) == GUARD
        hc, ha = np.full(n + 1, GUARD, dtype=np.uint32), np.full(n + 1, GUARD, dtype=np.uint32)
        raw_reflect(scene, ORIGINAL, info, lights, lights_ref.AMBIENT, rays, n, hc, None, ha, False, False, 96, 1, 96, 3)
        assert_words(hc[:n], want[:n], f"n = {n} on the host")
        assert_words(ha[:n], want_ao[:n], f"n = {n} ao on the host")
        assert int(hc[n]) == GUARD and int(ha[n]) == GUARD
    # the first ray of the slice alone, where it reflects: a list of one
    first = int(np.flatnonzero(want != plain)[0])
    dc = torch.full((2,), GUARD, dtype=torch.int32, device="cuda")
    raw_reflect(scene, ORIGINAL, info, lights, lights_ref.AMBIENT, drays[first:first + 1].contiguous(), 1, dc, None, None, True, True,
                96, 1, 96, 3)
    assert int(dc[0]) & 0xFFFFFFFF == int(want[first]) and int(dc[1]) == GUARD


# ---------------------------------------------------------------- (h) refusals on the device

def test_refusals_on_the_device_keep_the_buffers(golden_scenes):
    scene = golden_scenes[VCS]
    info = vr.VoxelSceneInfo(ZERO, SCALE)
    n = 67
    rays = np.ascontiguousarray(lights_cases.frame_rays()[300:300 + n])
    drays = device_rays(rays)
    lights = gpu_lights()
    dc = torch.full((n + 1,), GUARD, dtype=torch.int32, device="cuda")
    dh = torch.full((n + 1, 16), GUARD, dtype=torch.int32, device="cuda")
    da = torch.full((n + 1,), GUARD, dtype=torch.int32, device="cuda")
    args = dict(strength=96, apply=0, k=200, bounces=2)

    def call(r=drays, c=dc, h=dh, a=da):
        raw_reflect(scene, ORIGINAL, info, lights, lights_ref.AMBIENT, r, n, c, h, a, True, True, **args)

    for kw in (dict(r=drays.data_ptr() + 4), dict(c=dc.data_ptr() + 2), dict(h=dh.data_ptr() + 8), dict(a=da.data_ptr() + 1)):
        with pytest.raises(vr.VrError) as e:
            call(**kw)
        assert e.value.code == -1 and "vr_shade_lights_reflect" in str(e.value) and "aligned" in str(e.value)
    hits = device_records(ao_cases.frame_records(int(VCS), False)[300:300 + n])
    dout = torch.full((n + 1, 8), GUARD, dtype=torch.int32, device="cuda")
    for kw in (dict(rays=drays.data_ptr() + 4), dict(hits=hits.data_ptr() + 8), dict(out=dout.data_ptr() + 12)):
        a = dict(rays=drays, hits=hits, out=dout)
        a.update(kw)
        with pytest.raises(vr.VrError) as e:
            raw_bounce_rays(info, a["rays"], a["hits"], n, a["out"], True, True)
        assert e.value.code == -1 and "vr_bounce_rays" in str(e.value) and "aligned" in str(e.value)
    # a stream that is capturing a graph: refused before anything is enqueued (as vr_pick's test)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    errs = []
    with torch.cuda.graph(g, stream=s):
        for fn in (call, lambda: raw_bounce_rays(info, drays, hits, n, dout, True, True)):
            try:
                fn()
            except vr.VrError as e:
                errs.append(e)
    assert len(errs) == 2 and all(e.code == -1 and "captur" in str(e) for e in errs)
    assert "vr_shade_lights_reflect" in str(errs[0]) and "vr_bounce_rays" in str(errs[1])
    torch.cuda.synchronize()
    assert bool((dc == GUARD).all()) and bool((dh == GUARD).all()) and bool((da == GUARD).all()) and bool((dout == GUARD).all())
    call()
    assert_words(dc[:n], reflect_cases.golden_words(int(VCS), False, 200, 2, strength=96, apply=ao_ref.AMBIENT)[300:300 + n],
                 "after the refusals")
    assert dh[:n].cpu().numpy().tobytes() == ao_cases.frame_records(int(VCS), False)[300:300 + n].tobytes()
    assert int(dc[n]) == GUARD and bool((dh[n] == GUARD).all()) and int(da[n]) == GUARD


# ---------------------------------------------------------------- (i) learned state

def test_reflect_is_not_a_render_launch(golden_scenes):
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
    i = np.arange(w * h)
    rays = vr.camera_rays(cam, w, h, (i % w).astype(np.uint32), (i // w).astype(np.uint32))
    vr.forget_orders(0)
    bad, first, d = render_learned(scene, ORIGINAL, cam, lit, info, w, h, 0, h, want, None, 0)
    assert not bad, diff_report(first, want, w)
    uses = vr.debug_order_uses(0)
    for order in ORDERS:
        vr.shade_lights(scene, ORIGINAL, info, [lit], rays, ambient=lights_ref.AMBIENT, order=order, reflect=128, bounces=4, ao=96,
                        hits=True, return_ao=True)
        vr.shade_lights(scene, ORIGINAL, info, [lit], device_rays(rays), reflect=255, bounces=2, mirror=reflect_cases.BIT, order=order)
    recs = vr.trace(scene, ORIGINAL, info, rays)
    vr.bounce_rays(rays, recs, info)
    assert vr.debug_order_uses(0)["launches"] == uses["launches"]
    assert vr.debug_order_uses(0) == uses      # (not a render launch: no counter moves)
    bad, first, d = render_learned(scene, ORIGINAL, cam, lit, info, w, h, 0, h, want, None, 0, launches=3)
    assert not bad, diff_report(first, want, w)
    assert d["lane_order_uses"] == 3 and d["work_order_uses"] == 3 and d["lane_orders_made"] == 0 and \
        d["work_orders_made"] == 0, d
