"""CPU tests of the mirror-reflection arithmetic (csrc/vr_reflect_math.h) through bin/reflect_check,
in the manner of tests/test_ao_check.py: the tool's own checks pass (mix against the closed form for
all 256^3 byte triples and for packed words, the bounce's landmarks), and its bounce is byte for
byte tests/reflect_ref.bounce on the golden frame's records and on made-up records no walk writes."""
from __future__ import annotations

import os
import subprocess

import numpy as np

from tests import ao_cases, lights_cases, reflect_cases, reflect_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "voxelraymarcher_amd", "bin", "reflect_check")


def tool_bounce(rays, recs, scale, translation) -> np.ndarray:
    t = np.asarray(translation, dtype=np.float32).view(np.uint32)
    lines = ["%08x %08x %08x %d" % (int(t[0]), int(t[1]), int(t[2]), int(scale))]
    lines += [a.tobytes().hex() + " " + b.tobytes().hex() for a, b in zip(rays, recs)]
    r = subprocess.run([TOOL, "--bounce"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.split()
    assert len(out) == len(rays)
    return np.frombuffer(bytes.fromhex("".join(out)), dtype=reflect_ref.RAY_DTYPE)


def test_the_tools_own_checks_pass():
    r = subprocess.run([TOOL], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert subprocess.run([TOOL, "--nonsense"], capture_output=True, timeout=60).returncode == 2


def test_mix_matches_the_reference():
    rng = np.random.default_rng(3)
    a, b = rng.integers(0, 1 << 32, 4000, dtype=np.uint64).astype(np.uint32), rng.integers(0, 1 << 32, 4000, dtype=np.uint64).astype(np.uint32)
    for k in (0, 1, 96, 127, 128, 254, 255):
        got = reflect_ref.mix(a, b, k)
        assert (got >> 24 == 0).all()
        for sh in (16, 8, 0):
            A, B = ((a >> sh) & 0xFF).astype(np.int64), ((b >> sh) & 0xFF).astype(np.int64)
            # the nearest integer to (A (255 - k) + B k) / 255, halves up (no half occurs: 255 is odd)
            want = np.floor((A * (255 - k) + B * k) / 255.0 + 0.5).astype(np.int64)
            assert np.array_equal((got >> sh) & 0xFF, want)
    assert np.array_equal(reflect_ref.mix(a, b, 0), a & 0xFFFFFF) and np.array_equal(reflect_ref.mix(a, b, 255), b & 0xFFFFFF)


def test_bounce_on_the_golden_frames_records():
    rays = lights_cases.frame_rays()
    for store, longest in reflect_cases.PAIRS:
        recs = ao_cases.frame_records(store, longest)
        assert np.count_nonzero(recs["status"] == reflect_ref.VOXEL) >= 550
        for scale, tr in ((lights_cases.SCALE, (0.0, 0.0, 0.0)), (3, (-3.5, 4.5, -6.5))):
            want = reflect_ref.bounce(rays, recs, scale, tr)
            assert tool_bounce(rays, recs, scale, tr).tobytes() == want.tobytes(), (store, longest, scale)


def test_bounce_on_made_up_records():
    rays, recs = reflect_cases.made_up()
    axes = reflect_ref.axes_of(recs)
    # what the records claim to hold: every axis and sign, records without a bounce for each reason
    assert set(axes.tolist()) == {-1, 0, 1, 2} and np.count_nonzero(axes >= 0) >= 40
    assert set(recs["status"].tolist()) >= {0, 1, 2, 3, 4, 0xFFFFFFFF}
    voxel = recs[recs["status"] == reflect_ref.VOXEL]
    assert np.count_nonzero(reflect_ref.axes_of(voxel) < 0) >= 14          # normals that are none in VOXEL records
    assert recs["region"].min() == -2**31 and recs["region"].max() == 2**31 - 1
    assert recs["voxel"].min() == -2**31 and recs["voxel"].max() == 2**31 - 1
    live = axes >= 0
    assert np.isnan(recs["point"][live]).any() and np.isinf(recs["point"][live]).any()
    d = rays["direction"][live]
    assert np.isnan(d).any() and np.isinf(d).any() and (np.signbit(d) & (d == 0)).any()
    for scale, tr in reflect_cases.MADE_UP_FORMS:
        want = reflect_ref.bounce(rays, recs, scale, tr)
        assert tool_bounce(rays, recs, scale, tr).tobytes() == want.tobytes(), (scale, tr)
        w = want.view(np.uint32).reshape(-1, 8)
        assert (w[:, 3] == 0).all() and (w[:, 7] == 0).all()
        assert (w[~live][:, [0, 1, 2, 4, 5, 6]] == reflect_ref.QUIET_NAN).all()
        # the direction: one sign bit flipped on the axis, everything else as it came
        din = np.ascontiguousarray(rays["direction"]).view(np.uint32)[live]
        flipped = w[live][:, 4:7] ^ din
        assert (flipped[np.arange(len(flipped)), axes[live]] == 0x80000000).all() and (flipped.sum(axis=1) == 0x80000000).all()
    assert {s for s, _ in reflect_cases.MADE_UP_FORMS} >= {1, 3, 12}
