"""vr_atmosphere_apply and vr_shade_lights_atmosphere on the GPU, word for word against tests/atmos_ref.py,
for both stores and both algorithms:

 (a) the golden frame (tests/atmos_cases.py): bounces 0, 1 and 4, reflectivity 255 and 96, flags SKY,
     FOG and both, the three occlusion settings of tests/test_gpu_reflect.py, every order, host arrays
     and device tensors; hits and the occlusion values byte-identical to the plain call's;
 (b) atmosphere=None and flags 0 are shade_lights(reflect=...);
 (c) the call equals the fold, in torch integer ops, of shade_lights(hits=True), atmosphere_apply and
     bounce_rays per depth;
 (d) atmosphere_apply's bytes on the golden and on made-up records, in place, odd sizes with a guard
     word in the three stagings;
 (e) the mirror corridor, where no ray misses: the fog shows at every depth, the sky nowhere;
 (f) a painted key colour (some rays reflect, some do not) and lattice rays at scale 3 with a
     translation (bounce_origin's rounding is in the distance);
 (g) refusals on the device keep the buffers; (h) nothing learned or forgotten;
 (i) render_lights(atmosphere=..., samples=2) and the CLI's --sky / --fog frame.

Every test here needs the new entry points."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import ao_cases, atmos_cases, atmos_ref, lattice_cases, lights_cases, lights_ref, reflect_cases, reflect_ref
from tests.test_gpu_reflect import (AOS, GUARD, ORDERS, PAIR_ID, PAIRS, assert_words, device_rays, device_records, golden_scenes,  # noqa: F401
                                    gpu_lights, torch_mix, words)
from tests.test_png import decode_png

pytestmark = pytest.mark.gpu

vr = pytest.importorskip("voxelraymarcher_amd")
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "voxelraymarcher_amd", "bin", "VoxelRaymarcher")

VCS, HASH = vr.StorageType.VOXEL_CLUSTER_STORE, vr.StorageType.HASH_TABLE
ORIGINAL, LONGEST = vr.RayMarchAlgorithm.ORIGINAL, vr.RayMarchAlgorithm.LONGEST_AXIS
ZERO = (0.0, 0.0, 0.0)
W, H, SCALE = atmos_cases.W, atmos_cases.H, atmos_cases.SCALE
SKY, FOG = atmos_ref.SKY, atmos_ref.FOG
ATM = atmos_cases.ATMOSPHERE


def gpu_atm(a, flags=None):
    """The vr.Atmosphere of an atmos_ref.Atmosphere (with other flags)."""
    return vr.Atmosphere(a.zenith, a.horizon, a.nadir, a.up, a.fog_color, a.fog_start, a.fog_end, a.flags if flags is None else flags)


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
    records = ao_cases.frame_records(int(store), longest)
    want_ao = ao_cases.frame_ao(int(store), longest)
    for bounces in (0, 1, 4):
        for k in (255, 96):
            for kw_ao, strength, apply in AOS:
                plain = reflect_cases.golden_words(int(store), longest, k, bounces, strength=strength, apply=apply)
                for flags in atmos_cases.FLAGS:
                    want = atmos_cases.golden_words(int(store), longest, flags, k, bounces, strength=strength, apply=apply)
                    assert np.count_nonzero(want != plain) >= 1
                    atm = gpu_atm(ATM, flags)
                    for order in ORDERS:
                        tag = f"{PAIR_ID(pair)} bounces={bounces} k={k} flags={flags} ao={strength} {order.name}"
                        kw = dict(ambient=lights_ref.AMBIENT, order=order, reflect=k, bounces=bounces, atmosphere=atm, **kw_ao)
                        assert_words(vr.shade_lights(scene, algo, info, lights, rays, **kw), want, tag)
                        assert_words(scene.shade_lights(algo, info, lights, drays, **kw), want, tag + " on the device")
                    # hits and the occlusion values are the plain call's, on either side
                    kw = dict(ambient=lights_ref.AMBIENT, reflect=k, bounces=bounces, atmosphere=atm, hits=True, **kw_ao)
                    if strength is None:
                        col, recs = vr.shade_lights(scene, algo, info, lights, rays, **kw)
                        dcol, drecs = vr.shade_lights(scene, algo, info, lights, drays, **kw)
                    else:
                        col, recs, ao = vr.shade_lights(scene, algo, info, lights, rays, return_ao=True, **kw)
                        dcol, drecs, dao = vr.shade_lights(scene, algo, info, lights, drays, return_ao=True, **kw)
                        assert_words(ao, want_ao, tag + " ao")
                        assert_words(dao, want_ao, tag + " ao on the device")
                    assert_words(col, want, tag + " with hits")
                    assert_words(dcol, want, tag + " on the device with hits")
                    assert recs.tobytes() == records.tobytes() and drecs.cpu().numpy().tobytes() == records.tobytes(), tag
    # without reflect=: the plain frame under the atmosphere (depth 0 alone)
    want = atmos_cases.golden_words(int(store), longest, SKY | FOG, 0, 0)
    assert_words(vr.shade_lights(scene, algo, info, lights, rays, ambient=lights_ref.AMBIENT, atmosphere=gpu_atm(ATM)), want, "no reflect=")
    # the other atmospheres: an up that is no axis with an inverted ramp, a step
    for other in (atmos_cases.TILTED, atmos_cases.STEP):
        want = atmos_cases.golden_words(int(store), longest, SKY | FOG, 96, 2, atm=other)
        got = vr.shade_lights(scene, algo, info, lights, drays, ambient=lights_ref.AMBIENT, reflect=96, bounces=2, atmosphere=gpu_atm(other))
        assert_words(got, want, "another atmosphere")


# ---------------------------------------------------------------- (b) the null case

@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_ID)
def test_no_atmosphere_or_no_flags_is_the_reflect_call(golden_scenes, pair):
    store, algo = pair
    scene = golden_scenes[store]
    info = vr.VoxelSceneInfo(ZERO, SCALE)
    rays = lights_cases.frame_rays()
    drays = device_rays(rays)
    lights = gpu_lights()
    for kw_ao, strength, apply in AOS:
        for k, bounces, mirror in ((96, 2, None), (255, 4, reflect_cases.BIT), (0, 1, None), (200, 0, None)):
            kw = dict(ambient=lights_ref.AMBIENT, reflect=k, bounces=bounces, mirror=mirror, hits=True, **kw_ao)
            plain, recs = vr.shade_lights(scene, algo, info, lights, rays, **kw)
            assert_words(plain, reflect_cases.golden_words(int(store), algo == LONGEST, k, bounces, mirror or reflect_cases.EVERY,
                                                           strength=strength, apply=apply), "the reflect call")
            for atm in (None, gpu_atm(ATM, 0)):
                tag = f"reflect={k} bounces={bounces} mirror={mirror} ao={strength} atmosphere={'flags 0' if atm else None}"
                c1, r1 = vr.shade_lights(scene, algo, info, lights, rays, atmosphere=atm, **kw)
                assert_words(c1, words(plain), tag)
                c2, r2 = vr.shade_lights(scene, algo, info, lights, drays, atmosphere=atm, **kw)
                assert_words(c2, words(plain), tag + " on the device")
                assert r1.tobytes() == recs.tobytes() and r2.cpu().numpy().tobytes() == recs.tobytes()
    # flags 0 without reflect= is shade_lights
    assert_words(vr.shade_lights(scene, algo, info, lights, rays, ambient=lights_ref.AMBIENT, atmosphere=gpu_atm(ATM, 0)),
                 ao_cases.frame_words(int(store), algo == LONGEST, None), "flags 0, no reflect=")
    with pytest.raises(vr.VrError) as e:
        vr.shade_lights(scene, algo, info, lights, rays, atmosphere=gpu_atm(ATM, 4))
    assert e.value.code == -1 and "vr_shade_lights_atmosphere" in str(e.value) and "flags" in str(e.value)
    with pytest.raises(TypeError):
        vr.shade_lights(scene, algo, info, lights, rays, atmosphere=(1, 2, 3))


# ---------------------------------------------------------------- (c) composition on the device

def composed(scene, algo, info, lights, drays, atm, k, bounces, mirror, **kw):
    """The call's words from the public calls it stands for: per depth shade_lights with hits over
    bounce_rays of the depth above and atmosphere_apply over its words, rays and records, masked by
    what is alive, folded from the back in torch integer ops (tests/test_gpu_reflect.composed with
    the atmosphere in its place)."""
    cols, refls = [], []
    alive = torch.ones(drays.shape[0], dtype=torch.bool, device=drays.device)
    cur = drays
    for j in range(bounces + 1):
        c, h = vr.shade_lights(scene, algo, info, lights, cur, hits=True, **kw)
        a = vr.atmosphere_apply(cur, h, c, info, atm)
        cols.append(torch.where(alive, a, torch.zeros_like(a)))
        alive = alive & (h[:, 0] == 1) & ((h[:, 1] & mirror[0]) == mirror[1])
        refls.append(alive)
        if j < bounces:
            cur = vr.bounce_rays(cur, h, info)
    out = cols[bounces]
    for j in range(bounces - 1, -1, -1):
        out = torch.where(refls[j], torch_mix(cols[j], out, k), cols[j])
    return out


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_ID)
def test_the_call_is_the_fold_of_its_public_parts(golden_scenes, pair):
    store, algo = pair
    scene = golden_scenes[store]
    info = vr.VoxelSceneInfo(ZERO, SCALE)
    drays = device_rays(lights_cases.frame_rays())
    lights = gpu_lights()
    for k, bounces, mirror, kw_ao, flags in ((128, 3, (0, 0), AOS[0][0], SKY | FOG), (255, 4, (1, 1), AOS[1][0], SKY),
                                             (37, 2, (0, 0), AOS[2][0], FOG), (96, 1, (0, 0), AOS[0][0], SKY | FOG)):
        kw = dict(ambient=lights_ref.AMBIENT, **kw_ao)
        atm = gpu_atm(ATM, flags)
        want = composed(scene, algo, info, lights, drays, atm, k, bounces, mirror, **kw)
        got = vr.shade_lights(scene, algo, info, lights, drays, reflect=k, bounces=bounces, mirror=mirror, atmosphere=atm, **kw)
        assert_words(got, words(want), f"{PAIR_ID(pair)} k={k} bounces={bounces} mirror={mirror} flags={flags}")


# ---------------------------------------------------------------- (d) atmosphere_apply's bytes

def raw_apply(info, atm, rays, hits, cin, n, out, in_dev, out_dev):
    def ptr(a):
        return ctypes.c_void_p(a if isinstance(a, int) else (a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data))
    vr._capi.check(vr.lib().vr_atmosphere_apply(0, ctypes.byref(atm.raw), vr._capi.f3(info.translation), int(info.scale), ptr(rays),
                                                ptr(hits), ptr(cin), n, int(in_dev), ptr(out), int(out_dev),
                                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "vr_atmosphere_apply")


def device_words(w):
    return torch.from_numpy(np.ascontiguousarray(w).view(np.int32).copy()).cuda()


def test_atmosphere_apply_bytes():
    rays = lights_cases.frame_rays()
    frame_w = np.random.default_rng(9).integers(0, 1 << 32, len(rays), dtype=np.uint64).astype(np.uint32)
    cases = [(rays, ao_cases.frame_records(st, lg), frame_w, SCALE, ZERO) for st, lg in reflect_cases.PAIRS]
    cases += [(rays, ao_cases.frame_records(1, True), frame_w, 3, lattice_cases.TRANSLATION)]
    cases += [reflect_cases.made_up() + (atmos_cases.made_up_words(),) + form for form in reflect_cases.MADE_UP_FORMS]
    for rr, recs, w, scale, tr in cases:
        info = vr.VoxelSceneInfo(tr, scale)
        dr, dh, dw = device_rays(rr), device_records(recs), device_words(w)
        for ref_atm in (ATM, atmos_cases.TILTED, atmos_cases.STEP):
            for flags in (0, SKY, FOG, SKY | FOG):
                want = atmos_ref.atmos(ref_atm.with_flags(flags), w, rr, recs, scale, tr)
                atm = gpu_atm(ref_atm, flags)
                got = vr.atmosphere_apply(rr, recs, w, info, atm)
                assert got.dtype == np.uint32
                assert_words(got, want, f"scale {scale} flags {flags}")
                dgot = vr.atmosphere_apply(dr, dh, dw, info, atm)
                assert dgot.is_cuda and dgot.dtype == torch.int32 and tuple(dgot.shape) == (len(rr),)
                assert_words(dgot, want, f"scale {scale} flags {flags} on the device")
                assert np.array_equal(words(dw), w)                      # (the input is left alone)
        # in place on the device: out == in
        want = atmos_ref.atmos(ATM, w, rr, recs, scale, tr)
        inplace = dw.clone()
        raw_apply(info, gpu_atm(ATM), dr, dh, inplace, len(rr), inplace, True, True)
        assert_words(inplace, want, f"scale {scale} in place")
        # (n, 6) rays
        six = np.concatenate([rr["origin"], rr["direction"]], axis=1)
        assert_words(vr.atmosphere_apply(six, recs, w, info, gpu_atm(ATM)), want, "(n, 6) rays")
        assert_words(vr.atmosphere_apply(torch.from_numpy(six).cuda(), dh, dw, info, gpu_atm(ATM)), want, "(n, 6) rays on the device")
    # odd sizes, with a guard word after the output, in every staging
    rr, recs = reflect_cases.made_up()
    w = atmos_cases.made_up_words()
    scale, tr = reflect_cases.MADE_UP_FORMS[2]
    info = vr.VoxelSceneInfo(tr, scale)
    atm = gpu_atm(ATM)
    want = atmos_ref.atmos(ATM, w, rr, recs, scale, tr)
    assert len(want) >= 257 and np.count_nonzero(want[:63] != w[:63]) >= 10
    dr, dh, dw = device_rays(rr), device_records(recs), device_words(w)
    hr, hh, hw = np.ascontiguousarray(rr), np.ascontiguousarray(recs), np.ascontiguousarray(w)
    for n in (1, 63, 64, 65, 257):
        dout = torch.full((n + 1,), GUARD, dtype=torch.int32, device="cuda")
        raw_apply(info, atm, dr, dh, dw, n, dout, True, True)
        assert_words(dout[:n], want[:n], f"n = {n} on the device")
        assert int(dout[n]) == GUARD
        hout = np.full(n + 1, GUARD, dtype=np.uint32)
        raw_apply(info, atm, hr, hh, hw, n, hout, False, False)
        assert_words(hout[:n], want[:n], f"n = {n} on the host")
        assert int(hout[n]) == GUARD
        dout.fill_(GUARD)
        raw_apply(info, atm, hr, hh, hw, n, dout, False, True)
        assert_words(dout[:n], want[:n], f"n = {n} from the host to the device")
        assert int(dout[n]) == GUARD
    with pytest.raises(TypeError):
        vr.atmosphere_apply(dr, recs, w, info, atm)
    with pytest.raises(ValueError):
        vr.atmosphere_apply(rr[:5], recs[:4], w[:5], info, atm)


# ---------------------------------------------------------------- (e) the mirror corridor

CORRIDOR_ATM = atmos_ref.Atmosphere(zenith=(0.1, 0.3, 0.9), horizon=(0.8, 0.7, 0.6), nadir=(0.35, 0.2, 0.05), up=(0.0, 0.0, 1.0),
                                    fog_color=(0.55, 0.6, 0.7), fog_start=5.0, fog_end=40.0)     # (the legs are 12 to 28 long)


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_ID)
def test_mirror_corridor(pair):
    store, algo = pair
    lv = reflect_cases.corridor_levels(int(store), algo == LONGEST)
    assert reflect_ref.alive_counts(lv) == [reflect_cases.CORRIDOR_N] * 5          # every ray hits at every depth
    assert all((l.recs["status"] == atmos_ref.VOXEL).all() for l in lv)            # no misses at any depth
    xyz, rgb = reflect_cases.corridor_voxels()
    rays = reflect_cases.corridor_rays()
    info = vr.VoxelSceneInfo(ZERO, 1)
    lights = gpu_lights(reflect_cases.CORRIDOR_LIGHTS)
    amb = reflect_cases.CORRIDOR_AMBIENT
    with vr.create_scene(xyz, rgb, store) as scene:
        for k in (128, 255):
            for bounces in (0, 1, 2, 3, 4):
                plain = reflect_ref.fold(lv, k, bounces)
                want = atmos_ref.fold(lv, CORRIDOR_ATM.with_flags(FOG), k, bounces, 1)
                assert np.count_nonzero(want != plain) >= 100, (k, bounces)      # the fog shows at every fold depth
                got = vr.shade_lights(scene, algo, info, lights, rays, ambient=amb, reflect=k, bounces=bounces,
                                      atmosphere=gpu_atm(CORRIDOR_ATM, FOG))
                assert_words(got, want, f"corridor FOG k={k} bounces={bounces}")
                got = vr.shade_lights(scene, algo, info, lights, rays, ambient=amb, reflect=k, bounces=bounces,
                                      atmosphere=gpu_atm(CORRIDOR_ATM, SKY))
                assert_words(got, plain, f"corridor SKY k={k} bounces={bounces}")   # the sky alone changes none
        kw_ao, strength, apply = AOS[1]
        got = vr.shade_lights(scene, algo, info, lights, rays, ambient=amb, reflect=128, bounces=4, atmosphere=gpu_atm(CORRIDOR_ATM), **kw_ao)
        assert_words(got, atmos_ref.fold(lv, CORRIDOR_ATM, 128, 4, 1, strength=strength, apply=apply), "corridor with ao")


# ---------------------------------------------------------------- (f) a key colour, roundings

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
        for k, bounces, flags, (kw_ao, strength, apply) in ((255, 1, SKY | FOG, AOS[0]), (96, 2, FOG, AOS[1]), (255, 2, SKY, AOS[2])):
            got = vr.shade_lights(scene, algo, info, gpu_lights(), rays, ambient=lights_ref.AMBIENT, reflect=k, bounces=bounces,
                                  mirror=reflect_cases.KEY_MIRROR, atmosphere=gpu_atm(ATM, flags), **kw_ao)
            want = atmos_ref.fold(lv, ATM.with_flags(flags), k, bounces, SCALE, strength=strength, apply=apply)
            assert np.count_nonzero(want != reflect_ref.fold(lv, k, bounces, strength, apply)) >= 20
            assert_words(got, want, f"painted mirrors k={k} bounces={bounces} flags={flags}")


LATTICE_ATM = atmos_ref.Atmosphere(zenith=(0.1, 0.3, 0.9), horizon=(0.8, 0.7, 0.6), nadir=(0.35, 0.2, 0.05), up=(0.0, 1.0, 0.0),
                                   fog_color=(0.55, 0.6, 0.7), fog_start=0.5, fog_end=20.0)      # (scale 3: the scene is 35 units wide)


@pytest.mark.parametrize("pair", [PAIRS[0], PAIRS[3]], ids=PAIR_ID)
def test_lattice_rays_at_scale_3_with_a_translation(pair):
    store, algo = pair
    form = "scale3"
    scale, tr = lattice_cases.FORMS[form]
    assert scale == 3 and tr != ZERO
    xyz, rgb = lattice_cases.scene_voxels()
    rays = np.array(lattice_cases.family_rays("lattice", form))
    info = vr.VoxelSceneInfo(tr, scale)
    lv = reflect_cases.lattice_levels(form, int(store), algo == LONGEST)
    # the fog's ramp is in use at both depths: the roundings of the hit point reach the words
    for l in lv[:2]:
        q = atmos_ref.fog_q(LATTICE_ATM, l.rays, l.recs, scale, tr)[l.recs["status"] == atmos_ref.VOXEL]
        assert np.count_nonzero((q > 0) & (q < 256)) >= 50
    with vr.create_scene(xyz, rgb, store) as scene:
        for k, flags, (kw_ao, strength, apply) in ((255, FOG, AOS[0]), (96, SKY | FOG, AOS[2])):
            got, recs = vr.shade_lights(scene, algo, info, gpu_lights(reflect_cases.LATTICE_LIGHTS), rays, ambient=lights_ref.AMBIENT,
                                        reflect=k, bounces=reflect_cases.LATTICE_BOUNCES, hits=True,
                                        atmosphere=gpu_atm(LATTICE_ATM, flags), **kw_ao)
            want = atmos_ref.fold(lv, LATTICE_ATM.with_flags(flags), k, 2, scale, tr, strength=strength, apply=apply)
            assert_words(got, want, f"{form} {PAIR_ID(pair)} k={k} flags={flags}")
            assert recs.tobytes() == lv[0].recs.tobytes()


# ---------------------------------------------------------------- (g) refusals on the device

def raw_atmosphere(scene, algo, info, lights, ambient, rays, n, colors, hits, ao_out, in_dev, out_dev, strength, apply, k, bounces, atm,
                   mirror=(0, 0), order=0):
    def ptr(a):
        if a is None:
            return None
        return ctypes.c_void_p(a if isinstance(a, int) else (a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data))
    block = (vr._capi.VrLighting * len(lights))(*lights)
    vr._capi.check(vr.lib().vr_shade_lights_atmosphere(
        scene.handle, int(algo), block, len(lights), vr._capi.f3(ambient), vr._capi.f3(info.translation), int(info.scale), ptr(rays),
        n, int(in_dev), ptr(colors), ptr(hits), int(out_dev), int(order), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream),
        strength, apply, ptr(ao_out), k, bounces, mirror[0], mirror[1], ctypes.byref(atm.raw)), "vr_shade_lights_atmosphere")


def test_refusals_on_the_device_keep_the_buffers(golden_scenes):
    scene = golden_scenes[VCS]
    info = vr.VoxelSceneInfo(ZERO, SCALE)
    n, start = 67, 300
    rays = np.ascontiguousarray(lights_cases.frame_rays()[start:start + n])
    drays = device_rays(rays)
    lights = gpu_lights()
    atm = gpu_atm(ATM)
    dc = torch.full((n + 1,), GUARD, dtype=torch.int32, device="cuda")
    dh = torch.full((n + 1, 16), GUARD, dtype=torch.int32, device="cuda")
    da = torch.full((n + 1,), GUARD, dtype=torch.int32, device="cuda")
    args = dict(strength=96, apply=0, k=200, bounces=2)

    def call(r=drays, c=dc, h=dh, a=da, at=atm):
        raw_atmosphere(scene, ORIGINAL, info, lights, lights_ref.AMBIENT, r, n, c, h, a, True, True, atm=at, **args)

    for kw in (dict(r=drays.data_ptr() + 4), dict(c=dc.data_ptr() + 2), dict(h=dh.data_ptr() + 8), dict(a=da.data_ptr() + 1)):
        with pytest.raises(vr.VrError) as e:
            call(**kw)
        assert e.value.code == -1 and "vr_shade_lights_atmosphere" in str(e.value) and "aligned" in str(e.value)
    for flags in (4, 7, 0x80000001):
        with pytest.raises(vr.VrError) as e:
            call(at=gpu_atm(ATM, flags))
        assert e.value.code == -1 and "vr_shade_lights_atmosphere" in str(e.value) and "flags" in str(e.value)
    hits = device_records(ao_cases.frame_records(int(VCS), False)[start:start + n])
    win = torch.full((n + 1,), 0x00123456, dtype=torch.int32, device="cuda")
    dout = torch.full((n + 1,), GUARD, dtype=torch.int32, device="cuda")
    for kw in (dict(rays=drays.data_ptr() + 4), dict(hits=hits.data_ptr() + 8), dict(cin=win.data_ptr() + 2), dict(out=dout.data_ptr() + 1)):
        a = dict(rays=drays, hits=hits, cin=win, out=dout)
        a.update(kw)
        with pytest.raises(vr.VrError) as e:
            raw_apply(info, atm, a["rays"], a["hits"], a["cin"], n, a["out"], True, True)
        assert e.value.code == -1 and "vr_atmosphere_apply" in str(e.value) and "aligned" in str(e.value)
    with pytest.raises(vr.VrError) as e:
        raw_apply(info, gpu_atm(ATM, 8), drays, hits, win, n, dout, True, True)
    assert e.value.code == -1 and "vr_atmosphere_apply" in str(e.value) and "flags" in str(e.value)
    # a stream that is capturing a graph: refused before anything is enqueued (as tests/test_gpu_reflect.py's test)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    errs = []
    with torch.cuda.graph(g, stream=s):
        for fn in (call, lambda: raw_apply(info, atm, drays, hits, win, n, dout, True, True)):
            try:
                fn()
            except vr.VrError as e:
                errs.append(e)
    assert len(errs) == 2 and all(e.code == -1 and "captur" in str(e) for e in errs)
    assert "vr_shade_lights_atmosphere" in str(errs[0]) and "vr_atmosphere_apply" in str(errs[1])
    torch.cuda.synchronize()
    assert bool((dc == GUARD).all()) and bool((dh == GUARD).all()) and bool((da == GUARD).all()) and bool((dout == GUARD).all())
    assert bool((win == 0x00123456).all())
    call()
    assert_words(dc[:n], atmos_cases.golden_words(int(VCS), False, SKY | FOG, 200, 2, strength=AOS[1][1], apply=AOS[1][2])[start:start + n],
                 "after the refusals")
    assert dh[:n].cpu().numpy().tobytes() == ao_cases.frame_records(int(VCS), False)[start:start + n].tobytes()
    assert int(dc[n]) == GUARD and bool((dh[n] == GUARD).all()) and int(da[n]) == GUARD
    raw_apply(info, atm, drays, hits, win, n, dout, True, True)
    want = atmos_ref.atmos(ATM, np.full(n, 0x00123456, dtype=np.uint32), rays, ao_cases.frame_records(int(VCS), False)[start:start + n], SCALE)
    assert_words(dout[:n], want, "vr_atmosphere_apply after the refusals")
    assert int(dout[n]) == GUARD and int(win[n]) == 0x00123456


# ---------------------------------------------------------------- (h) learned state

def test_atmosphere_is_not_a_render_launch(golden_scenes):
    """The vr_debug_order_uses counters do not move over the calls."""
    scene = golden_scenes[VCS]
    info = vr.VoxelSceneInfo(ZERO, SCALE)
    lit = vr.setup_constant_values()
    cam = vr.Camera.reference(W, H)
    out = torch.empty(W * H, dtype=torch.int32, device="cuda")
    for _ in range(2):
        vr.run_raymarching_kernel(scene, ORIGINAL, cam, lit, info, W, H, out=out)
    torch.cuda.synchronize()
    uses = vr.debug_order_uses(0)
    assert uses["launches"] >= 2
    rays = lights_cases.frame_rays()
    for order in ORDERS:
        col, recs, _ = vr.shade_lights(scene, ORIGINAL, info, [lit], rays, ambient=lights_ref.AMBIENT, order=order, reflect=128, bounces=4,
                                       ao=96, hits=True, return_ao=True, atmosphere=gpu_atm(ATM))
        vr.shade_lights(scene, ORIGINAL, info, [lit], device_rays(rays), reflect=255, bounces=2, order=order, atmosphere=gpu_atm(ATM, FOG))
    vr.atmosphere_apply(rays, recs, col, info, gpu_atm(ATM))
    assert vr.debug_order_uses(0) == uses      # (not a render launch: no counter moves)


# ---------------------------------------------------------------- (i) frames

@pytest.mark.parametrize("pair", [PAIRS[0], PAIRS[3]], ids=PAIR_ID)
def test_render_lights_with_an_atmosphere(golden_scenes, pair):
    store, algo = pair
    scene = golden_scenes[store]
    longest = algo == LONGEST
    info = vr.VoxelSceneInfo(ZERO, SCALE)
    cam = vr.Camera.reference(W, H)
    atm = gpu_atm(ATM)
    for kw_ao, strength, apply in AOS[:2]:
        frame = vr.render_lights(scene, algo, cam, info, gpu_lights(), W, H, ambient=lights_ref.AMBIENT, reflect=96, bounces=2,
                                 atmosphere=atm, **kw_ao)
        assert frame.is_cuda and frame.dtype == torch.int32 and tuple(frame.shape) == (H, W)
        assert_words(frame.reshape(-1), atmos_cases.golden_words(int(store), longest, SKY | FOG, 96, 2, strength=strength, apply=apply),
                     f"render_lights ao={strength}")
    frame = vr.render_lights(scene, algo, cam, info, gpu_lights(), W, H, ambient=lights_ref.AMBIENT, atmosphere=atm)
    assert_words(frame.reshape(-1), atmos_cases.golden_words(int(store), longest, SKY | FOG, 0, 0), "render_lights, no reflect=")
    # samples=: the atmosphere passes through to the fine frame unchanged, which the filter resolves
    w, h = 13, 9
    args = (scene, algo, vr.Camera.reference(2 * w, 2 * h), info, gpu_lights(), 2 * w, 2 * h)
    fine = vr.render_lights(*args, ambient=lights_ref.AMBIENT, reflect=128, bounces=2, atmosphere=atm)
    plain = vr.render_lights(*args, ambient=lights_ref.AMBIENT, reflect=128, bounces=2)
    assert int((fine != plain).sum()) >= 100
    got = vr.render_lights(scene, algo, vr.Camera.reference(w, h), info, gpu_lights(), w, h, ambient=lights_ref.AMBIENT,
                           reflect=128, bounces=2, atmosphere=atm, samples=2)
    assert torch.equal(got, vr.resolve(fine, w, h, 2))


def cli_atmosphere(sky=None, fog=None):
    """The vr.Atmosphere the CLI makes of --sky / --fog: a byte b is the float (b + 0.5) / 255."""
    def channels(rgb):
        return tuple((((rgb >> sh) & 0xFF) + 0.5) / 255.0 for sh in (16, 8, 0))
    kw = {}
    if sky is not None:
        kw.update(zenith=channels(sky[0]), horizon=channels(sky[1]), nadir=channels(sky[2]))
    if fog is not None:
        kw.update(fog_color=channels(fog[0]), fog_start=fog[1], fog_end=fog[2])
    return vr.Atmosphere(flags=(SKY if sky is not None else 0) | (FOG if fog is not None else 0), **kw)


@pytest.mark.parametrize("store,algo", [("vcs", "original"), ("hashtable", "longestaxis")])
def test_cli_sky_and_fog_frame(tmp_path, store, algo):
    """`VoxelRaymarcher ... --sky ZZZZZZ,HHHHHH,NNNNNN --fog RRGGBB,START,END` writes the
    vr_shade_lights_atmosphere frame and extends its "lights" line."""
    xyz, rgb = lights_cases.golden_voxels()
    scene_path = str(tmp_path / "scene.vox")
    vr.write_voxel_file(scene_path, xyz, rgb)
    out = str(tmp_path / "output.png")
    base = [EXE, str(SCALE), store, algo, "--scene", scene_path, "--width", str(W), "--height", str(H), "--out", out]
    sky, fog = (0x1A4DE6, 0xCCB399, 0x59330D), (0x8C99B3, 0.25, 4.0)

    def png_words():
        px = decode_png(open(out, "rb").read()).astype(np.uint32)
        return (px[..., 0] << 16 | px[..., 1] << 8 | px[..., 2]).reshape(-1)

    # the colour bytes come back as given
    atm = cli_atmosphere(sky, fog)
    assert [atmos_ref.pack(tuple(c)) for c in (atm.raw.zenith, atm.raw.horizon, atm.raw.nadir, atm.raw.fog_color)] == list(sky) + [fog[0]]
    with vr.create_scene(xyz, rgb, vr.parse_storage(store)) as scene:
        args = (scene, vr.parse_algorithm(algo), vr.Camera.reference(W, H), vr.VoxelSceneInfo(ZERO, SCALE), [vr.setup_constant_values()], W, H)
        plain = vr.render_lights(*args)
        both = vr.render_lights(*args, ambient=(0.25, 0.25, 0.25), ao=96, reflect=96, bounces=3, atmosphere=atm)
        sky_only = vr.render_lights(*args, atmosphere=cli_atmosphere(sky=sky))
        fog_aa = vr.render_lights(*args, reflect=200, bounces=2, atmosphere=cli_atmosphere(fog=fog), samples=2)
    assert int((sky_only != plain).sum()) >= 170
    r = subprocess.run(base + ["--ambient", "0.25,0.25,0.25", "--ao", "96", "--reflect", "96", "--bounces", "3", "--sky",
                               "1a4de6,ccb399,59330d", "--fog", "8c99b3,0.25,4.0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ("lights 1 ambient 0.25 0.25 0.25 ao 96 ambient reflect 96 bounces 3 mirror every sky 1a4de6 ccb399 59330d fog 8c99b3 0.25 4"
            in r.stdout.splitlines())
    assert_words(png_words(), words(both.reshape(-1)), "--sky --fog with --reflect")
    # --sky alone selects the lights frame
    r = subprocess.run(base + ["--sky", "1A4DE6,CCB399,59330D"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "lights 1 ambient 0 0 0 sky 1a4de6 ccb399 59330d" in r.stdout.splitlines()
    assert_words(png_words(), words(sky_only.reshape(-1)), "--sky")
    # --fog with --reflect and --aa: the fine frame, resolved
    r = subprocess.run(base + ["--fog", "8c99b3,0.25,4", "--reflect", "200", "--bounces", "2", "--aa", "2"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "lights 1 ambient 0 0 0 reflect 200 bounces 2 mirror every fog 8c99b3 0.25 4" in r.stdout.splitlines()
    assert_words(png_words(), words(fog_aa.reshape(-1)), "--fog with --aa")
    # refusals need no device work
    for extra, word in ((["--sky", "ffffff,000000"], "--sky needs"), (["--sky", "ffffff,000000,zz"], "--sky needs"),
                        (["--sky", "ffffff,000000,1234567"], "--sky needs"), (["--sky", "ffffff,,000000"], "--sky needs"),
                        (["--sky", "1,2,3,4"], "--sky needs"), (["--fog", "ffffff,1"], "--fog needs"),
                        (["--fog", "ffffff,1,x"], "--fog needs"), (["--fog", "gg,1,2"], "--fog needs"),
                        (["--fog", "ffffff,1,2,3"], "--fog needs"), (["--fog", "ffffff,,2"], "--fog needs"),
                        (["--sky", "1,2,3", "--gpus", "2"], "--gpus"), (["--fog", "1,2,3", "--gpus", "2"], "--gpus")):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and word in r.stderr, r.stdout + r.stderr
