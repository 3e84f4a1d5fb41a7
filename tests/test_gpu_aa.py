"""vr_resolve and vr_render_aa on the GPU: supersampled, box-filtered frames.

The filter is held to tests/aa_ref.py on seeded random words for every sample count, sizes that
take each of its paths (odd widths, a lone pixel, one row, rows that are no multiple of a wave,
several workgroups), every combination of outputs, a fine buffer that is only 4-byte aligned, and
guard words around the outputs.  vr_render_aa is held to the oracle's own bigger render, box-filtered
(aa_ref.aa_frame): four store x algorithm pairs, a point light with shadows, a translation and a
scale, row ranges, under learned orders; render_lights(samples=) and the CLI's --aa write the same
words; a capturing stream is refused."""
from __future__ import annotations

import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle
from tests import aa_ref, fuzz_cases, lights_cases, lights_ref, shade_ref
from tests.helpers import diff_report, full_lane_blocks, gpu_render, oracle_camera_from, oracle_lighting_from
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
ZERO = (0.0, 0.0, 0.0)
W, H, SCALE = lights_cases.W, lights_cases.H, lights_cases.SCALE
GUARD = 64                       # guard words on each side of an output
PATTERN = 0x5A5A5A5A


def words_of(t) -> np.ndarray:
    return t.detach().cpu().numpy().reshape(-1).view(np.uint32)


def to_device(words: np.ndarray):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).cuda()


def rgb8_of(words: np.ndarray) -> np.ndarray:
    return np.stack([(words >> 16) & 0xFF, (words >> 8) & 0xFF, words & 0xFF], axis=1).astype(np.uint8).reshape(-1)


@pytest.fixture(scope="module")
def golden_scenes():
    """The golden scene per store on the GPU and in the oracle, built once."""
    xyz, rgb = lights_cases.golden_voxels()
    made = {s: (vr.create_scene(xyz, rgb, s), oracle.Scene(xyz, rgb, int(s))) for s in (VCS, HASH)}
    yield made
    for g, o in made.values():
        g.close()
        o.close()


@functools.lru_cache(maxsize=None)
def golden_want(store, algo, S, lighting="directional"):
    """(the oracle's fine frame, its resolved frame) of the golden view, read-only."""
    xyz, rgb = lights_cases.golden_voxels()
    sc = oracle.Scene(xyz, rgb, int(store))
    lit = shade_ref.fill_block(oracle.lighting(), *shade_ref.LIGHTINGS[lighting])
    fine = aa_ref.fine_frame(sc, int(algo), oracle.reference_camera(W, H), lit, W, H, S, SCALE)
    sc.close()
    want = aa_ref.resolve(fine, W, H, S)
    fine.setflags(write=False)
    want.setflags(write=False)
    return fine, want


# ---------------------------------------------------------------- 1. the filter on seeded words

SHAPES = [(1, 1), (3, 2), (5, 3), (64, 1), (67, 5), (130, 3), (32, 24)]


def seeded_fine(S, w, rows):
    """Random 32-bit words (most are >= 2^24); every third pixel row all 0xFFFFFF, the next all 0."""
    rng = np.random.default_rng(1000 * S + 10 * w + rows)
    fine = rng.integers(0, 1 << 32, size=(rows, S, S * w), dtype=np.uint32)
    if rows >= 3:
        fine[1::3] = 0x00FFFFFF
        fine[2::3] = 0
    assert (fine >> 24).any()
    return fine.reshape(-1)


def guarded(n, dtype):
    """A buffer of n elements between GUARD words of PATTERN on each side: (buffer, the middle)."""
    per = 4 if dtype == torch.uint8 else 1
    buf = torch.full((n + 2 * GUARD * per,), PATTERN & 0xFF if dtype == torch.uint8 else PATTERN, dtype=dtype, device="cuda")
    return buf, buf[GUARD * per:GUARD * per + n]


def guards_intact(buf, n, dtype) -> bool:
    per = 4 if dtype == torch.uint8 else 1
    g = GUARD * per
    val = PATTERN & 0xFF if dtype == torch.uint8 else PATTERN
    return bool((buf[:g] == val).all()) and bool((buf[g + n:] == val).all())


@pytest.mark.parametrize("S", aa_ref.SAMPLES)
def test_resolve_is_the_reference(S):
    for w, rows in SHAPES:
        fine = seeded_fine(S, w, rows)
        want = aa_ref.resolve(fine, w, rows, S)
        want_rgb = rgb8_of(want)
        aligned = to_device(fine)
        shifted = torch.empty(fine.size + 1, dtype=torch.int32, device="cuda")[1:]
        shifted.copy_(aligned)
        assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4
        for name, dfine in (("aligned", aligned), ("4 bytes past a 16-byte boundary", shifted)):
            n = w * rows
            for mode in ("words", "rgb8", "both"):
                tag = f"S={S} {w}x{rows} {name} {mode}"
                wbuf, wout = guarded(n, torch.int32)
                rbuf, rout = guarded(3 * n, torch.uint8)
                if mode == "words":
                    got = vr.resolve(dfine, w, rows, S, out=wout)
                    assert got is wout
                elif mode == "rgb8":
                    got = vr.resolve(dfine, w, rows, S, rgb8=rout)
                    assert got is rout
                else:
                    got = vr.resolve(dfine, w, rows, S, rgb8=rout, out=wout)
                    assert got[0] is wout and got[1] is rout
                torch.cuda.synchronize()
                if mode != "rgb8":
                    assert np.array_equal(words_of(wout), want), tag + ": " + diff_report(words_of(wout), want, w)
                else:
                    assert bool((wout == PATTERN).all()), tag
                if mode != "words":
                    assert np.array_equal(rout.cpu().numpy(), want_rgb), tag
                    assert np.array_equal(rout.cpu().numpy(), vr.pack_rgb8(to_device(want)).cpu().numpy()), tag
                else:
                    assert bool((rout == (PATTERN & 0xFF)).all()), tag
                assert guards_intact(wbuf, n, torch.int32) and guards_intact(rbuf, 3 * n, torch.uint8), tag
                assert np.array_equal(words_of(dfine), fine), tag       # the fine frame is only read
        # the outputs the call allocates: (rows, w) words, (rows, w, 3) bytes
        out = vr.resolve(aligned, w, rows, S)
        rgb = vr.resolve(aligned, w, rows, S, rgb8=True)
        assert tuple(out.shape) == (rows, w) and out.dtype == torch.int32 and np.array_equal(words_of(out), want)
        assert tuple(rgb.shape) == (rows, w, 3) and rgb.dtype == torch.uint8
        assert np.array_equal(rgb.cpu().numpy().reshape(-1), want_rgb)


# ---------------------------------------------------------------- 2. vr_render_aa is the oracle's bigger render, filtered

@pytest.mark.parametrize("S", [2, 4, 8])
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_ID)
def test_render_aa_is_the_resolved_oracle_frame(golden_scenes, pair, S):
    store, algo = pair
    scene = golden_scenes[store][0]
    fine_want, want = golden_want(store, algo, S)
    fine = torch.full((vr.aa_fine_words(W, H, S),), -1, dtype=torch.int32, device="cuda")
    out, rgb = vr.render_aa(scene, algo, vr.Camera.reference(W, H), vr.setup_constant_values(), vr.VoxelSceneInfo(ZERO, SCALE),
                            W, H, S, fine=fine, out=torch.full((H * W,), -1, dtype=torch.int32, device="cuda"), rgb8=True)
    torch.cuda.synchronize()
    assert np.array_equal(words_of(out), want), diff_report(words_of(out), want, W)
    assert np.array_equal(words_of(fine), fine_want), diff_report(words_of(fine), fine_want, S * W)
    assert np.array_equal(rgb.cpu().numpy().reshape(-1), rgb8_of(want))
    # without a fine buffer of the caller's, and without `out`: the same words
    alone = vr.render_aa(scene, algo, vr.Camera.reference(W, H), vr.setup_constant_values(), vr.VoxelSceneInfo(ZERO, SCALE),
                         W, H, S)
    assert tuple(alone.shape) == (H, W) and np.array_equal(words_of(alone), want)


def test_render_aa_point_light_with_shadows(golden_scenes):
    spec = shade_ref.LIGHTINGS["point"]
    assert spec[0] and spec[1]                       # shadows, point light
    lit = shade_ref.fill_block(vr.setup_constant_values(), *spec)
    for S in (2, 4):
        fine_want, want = golden_want(VCS, ORIGINAL, S, "point")
        assert not np.array_equal(want, golden_want(VCS, ORIGINAL, S)[1])
        fine = torch.full((vr.aa_fine_words(W, H, S),), -1, dtype=torch.int32, device="cuda")
        out = vr.render_aa(golden_scenes[VCS][0], ORIGINAL, vr.Camera.reference(W, H), lit, vr.VoxelSceneInfo(ZERO, SCALE),
                           W, H, S, fine=fine)
        assert np.array_equal(words_of(out), want), diff_report(words_of(out), want, W)
        assert np.array_equal(words_of(fine), fine_want)


def test_render_aa_translation_and_scale():
    """A fuzz case with a translation, a scale, a point light and an odd width (at S = 2 the filter
    then reads word by word)."""
    c = fuzz_cases.make_case(1002)
    assert c.scale == 3 and any(c.translation) and c.W % 2 == 1
    cam = vr.Camera(c.eye, c.look_at, c.up, c.fov, c.aspect)
    lit = vr.setup_constant_values(use_shadows=c.shadows, use_point_light=c.point, light_position=c.light_pos,
                                   light_direction=c.light_dir, light_color=c.light_color)
    info = vr.VoxelSceneInfo(c.translation, c.scale)
    ref = oracle.Scene(c.xyz, c.rgb, int(HASH))
    with vr.create_scene(c.xyz, c.rgb, HASH) as scene:
        for S in (2, 4):
            fine_want = aa_ref.fine_frame(ref, int(LONGEST), oracle_camera_from(cam), oracle_lighting_from(lit), c.W, c.H, S,
                                          c.scale, translation=c.translation)
            want = aa_ref.resolve(fine_want, c.W, c.H, S)
            assert np.count_nonzero(want) >= 100
            fine = torch.full((vr.aa_fine_words(c.W, c.H, S),), -1, dtype=torch.int32, device="cuda")
            out = vr.render_aa(scene, LONGEST, cam, lit, info, c.W, c.H, S, fine=fine)
            assert np.array_equal(words_of(out), want), diff_report(words_of(out), want, c.W)
            assert np.array_equal(words_of(fine), fine_want)
    ref.close()


# ---------------------------------------------------------------- 3. row ranges, one sample

@pytest.mark.parametrize("pair", [(VCS, LONGEST), (HASH, ORIGINAL)], ids=PAIR_ID)
def test_row_ranges_are_slices_of_the_frame(golden_scenes, pair):
    store, algo = pair
    scene = golden_scenes[store][0]
    cam, lit, info = vr.Camera.reference(W, H), vr.setup_constant_values(), vr.VoxelSceneInfo(ZERO, SCALE)
    for S in (2, 4):
        fine_want, want = golden_want(store, algo, S)
        for r0, r1 in ((5, 17), (23, 24)):
            n = (r1 - r0) * W
            fine = torch.full((vr.aa_fine_words(W, r1 - r0, S) + 8,), -1, dtype=torch.int32, device="cuda")
            wbuf, wout = guarded(n, torch.int32)
            vr.render_aa(scene, algo, cam, lit, info, W, H, S, rows=(r0, r1), fine=fine, out=wout)
            torch.cuda.synchronize()
            tag = f"S={S} rows [{r0}, {r1})"
            assert np.array_equal(words_of(wout), want[r0 * W:r1 * W]), tag
            assert guards_intact(wbuf, n, torch.int32), tag
            fw = S * W * S
            assert np.array_equal(words_of(fine)[:-8], fine_want[r0 * fw:r1 * fw]), tag
            assert bool((fine[-8:] == -1).all()), tag
        # an empty range does nothing
        wbuf, wout = guarded(W, torch.int32)
        vr.render_aa(scene, algo, cam, lit, info, W, H, S, rows=(7, 7), out=wout[:0])
        torch.cuda.synchronize()
        assert bool((wbuf == PATTERN).all())
    # one sample per pixel: the render with bits 24-31 cleared
    one = vr.render_aa(scene, algo, cam, lit, info, W, H, 1)
    plain, _ = gpu_render(scene, algo, cam, lit, info, W, H)
    assert np.array_equal(words_of(one), plain & np.uint32(0xFFFFFF))
    assert np.array_equal(words_of(one), golden_want(store, algo, 1)[1])


# ---------------------------------------------------------------- 4. under learned orders

@pytest.mark.parametrize("pair", [(VCS, ORIGINAL), (HASH, LONGEST)], ids=PAIR_ID)
def test_repeated_view_renders_under_its_lane_order(golden_scenes, pair):
    """The fine view is an ordinary render launch: launched slots + 2 times it comes under its
    lane order (vr_debug_order_uses()[2] grows), and every frame is the oracle's."""
    store, algo = pair
    S = 4
    scene = golden_scenes[store][0]
    cam, lit, info = vr.Camera.reference(W, H), vr.setup_constant_values(), vr.VoxelSceneInfo(ZERO, SCALE)
    fine_want, want = golden_want(store, algo, S)
    device = scene.info()["device"]
    before = vr.debug_order_uses(device)
    assert full_lane_blocks(S * W, S * H, before["lane_block"]) >= 1
    fine = torch.empty(vr.aa_fine_words(W, H, S), dtype=torch.int32, device="cuda")
    out = torch.empty(H * W, dtype=torch.int32, device="cuda")
    launches = before["slots"] + 2
    for k in range(launches):
        fine.fill_(-1)
        out.fill_(-1)
        vr.render_aa(scene, algo, cam, lit, info, W, H, S, fine=fine, out=out)
        torch.cuda.synchronize()
        assert np.array_equal(words_of(out), want), f"launch {k}: " + diff_report(words_of(out), want, W)
        assert np.array_equal(words_of(fine), fine_want), f"launch {k}"
    after = vr.debug_order_uses(device)
    assert after["launches"] - before["launches"] == launches
    assert after["lane_order_uses"] > before["lane_order_uses"], (before, after)


# ---------------------------------------------------------------- 5. several lights

@pytest.mark.parametrize("pair", [(VCS, LONGEST), (HASH, ORIGINAL)], ids=PAIR_ID)
def test_render_lights_samples(golden_scenes, pair):
    store, algo = pair
    scene = golden_scenes[store][0]
    lights = [lights_ref.fill_block(vr.setup_constant_values(), l) for l in (lights_ref.LIGHT_A, lights_ref.LIGHT_B)]
    cam, info = vr.Camera.reference(W, H), vr.VoxelSceneInfo(ZERO, SCALE)
    fine = vr.render_lights(scene, algo, cam, info, lights, 2 * W, 2 * H, ambient=lights_ref.AMBIENT)
    assert tuple(fine.shape) == (2 * H, 2 * W)
    want = vr.resolve(fine, W, H, 2)
    got = vr.render_lights(scene, algo, cam, info, lights, W, H, ambient=lights_ref.AMBIENT, samples=2)
    assert tuple(got.shape) == (H, W) and torch.equal(got, want)
    assert np.array_equal(words_of(got), aa_ref.resolve(words_of(fine), W, H, 2))
    one = vr.render_lights(scene, algo, cam, info, lights, W, H, ambient=lights_ref.AMBIENT)
    assert torch.equal(vr.render_lights(scene, algo, cam, info, lights, W, H, ambient=lights_ref.AMBIENT, samples=1), one)
    assert int((got != one).sum()) >= 450          # the yardstick's floor at S = 2
    with pytest.raises(ValueError):
        vr.render_lights(scene, algo, cam, info, lights, W, H, samples=3)


# ---------------------------------------------------------------- 6. the CLI

@pytest.mark.parametrize("store,algo", [("vcs", "longestaxis"), ("hashtable", "original")])
def test_cli_aa_frame(tmp_path, store, algo):
    xyz, rgb = lights_cases.golden_voxels()
    scene_path = str(tmp_path / "scene.vox")
    vr.write_voxel_file(scene_path, xyz, rgb)
    out = str(tmp_path / "output.png")
    r = subprocess.run([EXE, str(SCALE), store, algo, "--scene", scene_path, "--width", str(W), "--height", str(H), "--out",
                        out, "--aa", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    want = golden_want(vr.parse_storage(store), vr.parse_algorithm(algo), 2)[1]
    got = decode_png(open(out, "rb").read())
    assert got.shape == (H, W, 3) and np.array_equal(got.reshape(-1), rgb8_of(want))
    # with an added light and an ambient term: the lights frame at twice the size, resolved
    r = subprocess.run([EXE, str(SCALE), store, algo, "--scene", scene_path, "--width", str(W), "--height", str(H), "--out",
                        out, "--aa", "2", "--add-light", "-2.0,1.0,3.0,0.5,0.75,1.0", "--ambient", "0.25,0.25,0.25"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lights = [vr.setup_constant_values(), vr.setup_constant_values(light_direction=(-2.0, 1.0, 3.0), light_color=(0.5, 0.75, 1.0))]
    with vr.create_scene(xyz, rgb, vr.parse_storage(store)) as scene:
        frame = vr.render_lights(scene, vr.parse_algorithm(algo), vr.Camera.reference(W, H), vr.VoxelSceneInfo(ZERO, SCALE),
                                 lights, W, H, ambient=(0.25, 0.25, 0.25), samples=2)
    got = decode_png(open(out, "rb").read())
    assert got.shape == (H, W, 3) and np.array_equal(got.reshape(-1), rgb8_of(words_of(frame)))


def test_cli_aa_refusals(tmp_path):
    base = [EXE, "1", "vcs", "original", "--synth", "64", "--width", "64", "--height", "64", "--out", str(tmp_path / "o.png")]
    r = subprocess.run(base + ["--aa", "3"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--aa needs 1, 2, 4 or 8" in r.stderr, r.stdout + r.stderr
    r = subprocess.run(base + ["--aa", "2", "--gpus", "1"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--aa" in r.stderr and "--gpus" in r.stderr, r.stdout + r.stderr
    r = subprocess.run(base + ["--aa"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--aa needs a value" in r.stderr
    assert not os.path.exists(tmp_path / "o.png")


# ---------------------------------------------------------------- 7. no graph capture

def test_capturing_stream_is_refused(golden_scenes):
    """vr_resolve and vr_render_aa on a stream that is capturing a graph return VR_E_INVALID before
    they enqueue anything; the capture ends cleanly and a frame after it is exact."""
    scene = golden_scenes[VCS][0]
    cam, lit, info = vr.Camera.reference(W, H), vr.setup_constant_values(), vr.VoxelSceneInfo(ZERO, SCALE)
    S = 2
    fine_want, want = golden_want(VCS, ORIGINAL, S)
    fine = torch.full((vr.aa_fine_words(W, H, S),), -1, dtype=torch.int32, device="cuda")
    out = torch.full((H * W,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    errs = []
    with torch.cuda.graph(g, stream=s):
        try:
            vr.render_aa(scene, ORIGINAL, cam, lit, info, W, H, S, fine=fine, out=out)
        except vr.VrError as e:
            errs.append(e)
        try:
            vr.resolve(fine, W, H, S, out=out)
        except vr.VrError as e:
            errs.append(e)
    assert len(errs) == 2 and all(e.code == -1 and "captur" in str(e) for e in errs)
    assert "vr_render_aa" in str(errs[0]) and "vr_resolve" in str(errs[1])
    torch.cuda.synchronize()
    assert bool((fine == -1).all()) and bool((out == -1).all())
    vr.render_aa(scene, ORIGINAL, cam, lit, info, W, H, S, fine=fine, out=out)
    assert np.array_equal(words_of(out), want) and np.array_equal(words_of(fine), fine_want)
