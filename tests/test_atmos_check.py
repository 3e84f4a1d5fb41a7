"""CPU tests of the atmosphere's arithmetic (csrc/vr_atmos_math.h) through bin/atmos_check, in the
manner of tests/test_reflect_check.py: the tool's own checks pass (lerp256 against the closed form for
every (A, B, q), q256's and the colour bytes' landmarks, landmarks of the sky and the fog), and its
atmos is byte for byte tests/atmos_ref.atmos on the golden frame's rays and records of all four pairs
(at depth 0 and, with the bounce rays, at depth 1) and on made-up records no walk writes, under every
combination of the flags."""
from __future__ import annotations

import os
import subprocess

import numpy as np

from tests import ao_cases, atmos_cases, atmos_ref, lights_cases, reflect_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "voxelraymarcher_amd", "bin", "atmos_check")
ALL_FLAGS = (0, atmos_ref.SKY, atmos_ref.FOG, atmos_ref.SKY | atmos_ref.FOG)
ATMOSPHERES = (atmos_cases.ATMOSPHERE, atmos_cases.TILTED, atmos_cases.STEP)


def tool_atmos(atm, w, rays, recs, scale, translation) -> np.ndarray:
    t = np.asarray(translation, dtype=np.float32).view(np.uint32)
    lines = ["%08x %08x %08x %d" % (int(t[0]), int(t[1]), int(t[2]), int(scale))]
    lines += [" ".join("%08x" % int(u) for u in atm.floats().view(np.uint32)) + " %d" % atm.flags]
    lines += [a.tobytes().hex() + " " + b.tobytes().hex() + " %08x" % int(c) for a, b, c in zip(rays, recs, w)]
    r = subprocess.run([TOOL, "--atmos"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.split()
    assert len(out) == len(rays)
    return np.array([int(x, 16) for x in out], dtype=np.uint32)


def test_the_tools_own_checks_pass():
    r = subprocess.run([TOOL], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert subprocess.run([TOOL, "--nonsense"], capture_output=True, timeout=60).returncode == 2


def test_the_references_pieces():
    # byte: truncation, the clamp, NaN and negatives
    assert [atmos_ref.byte(x) for x in (0.0, -1.0, float("nan"), 1.0, 2.0, float("inf"), 0.5, 0.25, 0.004)] == \
        [0, 0, 0, 255, 255, 255, 127, 63, 1]
    assert atmos_ref.pack((1.0, 0.5, 0.25)) == 0xFF7F3F
    # q256
    f = np.array([0.0, -0.0, 1e-45, 1.0 - 2.0 ** -24, 1.0, np.nan, np.inf, -np.inf, 0.5, 1.0 / 256, -0.5], dtype=np.float32)
    assert atmos_ref.q256(f).tolist() == [0, 0, 0, 255, 256, 0, 256, 0, 128, 1, 0]
    # lerp256 against the closed form: the nearest integer to (A (256 - q) + B q) / 256, halves up
    rng = np.random.default_rng(3)
    a = rng.integers(0, 1 << 32, 4000, dtype=np.uint64).astype(np.uint32)
    b = rng.integers(0, 1 << 32, 4000, dtype=np.uint64).astype(np.uint32)
    for q in (0, 1, 96, 127, 128, 129, 255, 256):
        got = atmos_ref.lerp256(a, b, q)
        assert (got >> 24 == 0).all()
        for sh in (16, 8, 0):
            A, B = ((a >> sh) & 0xFF).astype(np.int64), ((b >> sh) & 0xFF).astype(np.int64)
            want = np.floor((A * (256 - q) + B * q) / 256.0 + 0.5).astype(np.int64)      # (exact in float64)
            assert np.array_equal((got >> sh) & 0xFF, want)
    assert np.array_equal(atmos_ref.lerp256(a, b, 0), a & 0xFFFFFF) and np.array_equal(atmos_ref.lerp256(a, b, 256), b & 0xFFFFFF)


def test_atmos_on_the_golden_frames_records():
    rays = lights_cases.frame_rays()
    w = np.random.default_rng(9).integers(0, 1 << 24, len(rays), dtype=np.uint64).astype(np.uint32)
    for store, longest in reflect_cases.PAIRS:
        recs = ao_cases.frame_records(store, longest)
        assert np.count_nonzero(recs["status"] == atmos_ref.VOXEL) >= 550 and np.count_nonzero(recs["status"] == atmos_ref.MISS) >= 170
        deeper = reflect_cases.golden_levels(store, longest)[1]      # the bounce rays: origins on the voxels' faces
        for flags in ALL_FLAGS:
            for atm in ATMOSPHERES:
                atm = atm.with_flags(flags)
                want = atmos_ref.atmos(atm, w, rays, recs, lights_cases.SCALE)
                assert np.array_equal(tool_atmos(atm, w, rays, recs, lights_cases.SCALE, (0.0, 0.0, 0.0)), want), (store, longest, flags)
                if flags == 0:
                    assert np.array_equal(want, w)
            atm = atmos_cases.ATMOSPHERE.with_flags(flags)
            wd = w[: len(deeper.rays)]
            want = atmos_ref.atmos(atm, wd, deeper.rays, deeper.recs, lights_cases.SCALE)
            assert np.array_equal(tool_atmos(atm, wd, deeper.rays, deeper.recs, lights_cases.SCALE, (0.0, 0.0, 0.0)), want)
        # another form of the same records: scale 3 and a translation put the roundings of the hit point into D
        atm = atmos_cases.ATMOSPHERE
        want = atmos_ref.atmos(atm, w, rays, recs, 3, (-3.5, 4.5, -6.5))
        assert np.array_equal(tool_atmos(atm, w, rays, recs, 3, (-3.5, 4.5, -6.5)), want)


def test_atmos_on_made_up_records():
    rays, recs = reflect_cases.made_up()
    w = atmos_cases.made_up_words()
    assert set(recs["status"].tolist()) >= {0, 1, 2, 3, 4, 0xFFFFFFFF}
    voxel, miss = recs["status"] == atmos_ref.VOXEL, recs["status"] == atmos_ref.MISS
    assert np.isnan(recs["point"][voxel]).any() and np.isinf(recs["point"][voxel]).any()
    d = rays["direction"][miss]
    assert np.isnan(d).any() and np.isinf(d).any() and (d == 0).all(axis=1).any()
    for scale, tr in reflect_cases.MADE_UP_FORMS:
        for flags in ALL_FLAGS:
            for atm in ATMOSPHERES:
                atm = atm.with_flags(flags)
                want = atmos_ref.atmos(atm, w, rays, recs, scale, tr)
                assert np.array_equal(tool_atmos(atm, w, rays, recs, scale, tr), want), (scale, tr, flags)
                # every record that is neither a MISS under SKY nor a VOXEL record under FOG keeps its word, bits 24-31 too
                keep = ~((miss & bool(flags & atmos_ref.SKY)) | (voxel & bool(flags & atmos_ref.FOG)))
                assert np.array_equal(want[keep], w[keep]) and (want[~keep] >> 24 == 0).all()
    # a NaN h gives the horizon: the zero direction among the MISS records
    zero = miss & (rays["direction"] == 0).all(axis=1)
    sky = atmos_ref.sky(atmos_cases.ATMOSPHERE, rays)
    assert zero.any() and (sky[zero] == atmos_ref.pack(atmos_cases.ATMOSPHERE.horizon)).all()
