"""vr_occlusion's arithmetic (csrc/vr_occlusion_math.h) on a CPU, by the stand-alone program
csrc/tools/ao_check.cpp: its own checks (the corner rule for all 256 occupancy patterns against a
spelled-out table; the bilinear sum, the rounding, the factor and scale_rgb against plain loops),
and tests/ao_ref.py held to it on made-up records: every axis and sign, NaN and negative points,
q exactly 0 and 256, coordinates that wrap past INT32_MAX, records that are open by definition."""
from __future__ import annotations

import os
import subprocess

import numpy as np

from tests import ao_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "voxelraymarcher_amd", "bin", "ao_check")
INT32_MAX, INT32_MIN = 2**31 - 1, -2**31


def rec(status, voxel, normal, region, point):
    r = np.zeros((), dtype=ao_ref.HIT_DTYPE)
    r["status"], r["color"] = status, 0x808080
    r["voxel"], r["normal"], r["region"], r["point"] = voxel, normal, region, point
    return r


def test_the_programs_own_checks_pass():
    assert os.path.exists(EXE), "build with make -C voxelraymarcher_amd/csrc"
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr


def cases():
    """(voxel set, record) pairs."""
    nan = float("nan")
    # a step: a floor at y = 9 under x in 8..12, z in 8..12, a wall at x = 12, a pillar at (9, 10, 9)
    solid = [(x, 9, z) for x in range(8, 13) for z in range(8, 13)] + [(12, 10, z) for z in range(8, 13)] + [(9, 10, 9)]
    vox = ao_ref.voxel_set(solid)
    out = []
    for point in [(10.5, 10.0, 10.5), (10.0, 10.0, 10.0), (11.0, 10.0, 11.0), (10.99999, 10.0, 10.003), (10.25, 10.0, 10.75),
                  (nan, 10.0, 10.5), (10.5, 10.0, nan), (-3.0, 10.0, 10.5), (10.5, 10.0, -0.0), (99.0, 10.0, 1e30),
                  (10.00390625, 10.0, 10.99609375), (float("inf"), 10.0, float("-inf"))]:
        out.append((vox, rec(1, (10, 9, 10), (0, 1, 0), (0, 0, 0), point)))
        out.append((vox, rec(1, (11, 9, 9), (0, 1, 0), (0, 0, 0), point)))      # beside the wall
    # every axis and sign around a lone cross of voxels, with a point off the centre
    cross = ao_ref.voxel_set([(0, 0, 0), (1, 1, 0), (-1, 0, 1), (0, -1, -1), (1, 0, 1), (0, 1, 1), (-1, -1, 0), (1, -1, 1)])
    for n in [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]:
        out.append((cross, rec(1, (0, 0, 0), n, (0, 0, 0), (0.3, 0.6, 0.9))))
        out.append((cross, rec(1, (0, 0, 0), n, (-1, -1, -1), (64.3, 64.6, 64.9))))   # (a region the voxel is not in)
    # wrapped coordinates: INT32_MAX + 1 is INT32_MIN, in the plane cell and in a neighbour
    edge = ao_ref.voxel_set([(INT32_MIN, 5, 4), (INT32_MIN, 4, 5), (INT32_MAX, 6, 6), (INT32_MIN, INT32_MAX, INT32_MIN),
                             (5, INT32_MIN, INT32_MIN)])
    out.append((edge, rec(1, (INT32_MAX, 5, 5), (1, 0, 0), (33554431, 0, 0), (63.5, 5.5, 5.25))))
    out.append((edge, rec(1, (5, INT32_MAX, 5), (0, 0, 1), (0, 33554431, 0), (5.5, 63.5, 6.0))))
    out.append((edge, rec(1, (5, INT32_MAX, INT32_MAX), (0, 1, 0), (0, 33554431, 33554431), (5.5, 64.0, 63.25))))
    out.append((edge, rec(1, (INT32_MIN, INT32_MIN, INT32_MIN), (0, 0, -1), (-33554432, -33554432, -33554432), (0.5, 0.5, 0.0))))
    out.append((edge, rec(1, (INT32_MAX, 5, 5), (1, 0, 0), (INT32_MAX, INT32_MIN, 77), (1.0, 2.0, 3.0))))   # 64 * region wraps
    # open by definition
    for status in (0, 2, 3, 4, 0xFFFFFFFF):
        out.append((vox, rec(status, (10, 9, 10), (0, 1, 0), (0, 0, 0), (10.5, 10.0, 10.5))))
    for n in [(0, 0, 0), (1, 1, 0), (0, 2, 0), (1, 0, -1), (0, 0, INT32_MIN), (1, 1, 1)]:
        out.append((vox, rec(1, (10, 9, 10), n, (0, 0, 0), (10.5, 10.0, 10.5))))
    return out


def test_ao_ref_is_the_program_on_made_up_records():
    pairs = cases()
    details = [ao_ref.detail(v, r) for v, r in pairs]
    args = [EXE, "--records"]
    for (_, r), d in zip(pairs, details):
        args += [r.tobytes().hex(), "%02x" % (d["occ"] if d else 0)]
    out = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    got = [tuple(int(x) for x in ln.split()) for ln in out.stdout.splitlines()]
    want = [(d["axis"], d["qu"], d["qw"], d["ao"]) if d else (-1, 0, 0, 255) for d in details]
    assert len(got) == len(want)
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, f"record {bad[0]}: ao_check {got[bad[0]]} ao_ref {want[bad[0]]} ({pairs[bad[0]][1]})"
    assert [ao_ref.occlusion(v, np.array([r]))[0] for v, r in pairs] == [w[3] for w in want]
    # the cases cover what they are meant to: q exactly 0 and 256, clamps from NaN, negatives and
    # overflow, all three axes, occluded and open values, a wrapped neighbour that is stored
    live = [d for d in details if d]
    qs = {q for d in live for q in (d["qu"], d["qw"])}
    assert {0, 1, 128, 255, 256} <= qs and {d["axis"] for d in live} == {0, 1, 2}
    assert len({d["ao"] for d in live}) >= 10 and min(d["ao"] for d in live) < 100 and any(d["ao"] == 255 for d in live)
    wrapped = [d for (v, _), d in zip(pairs, details) if d and INT32_MIN in {c for t in v for c in t}]
    assert len(wrapped) == 5 and sum(d["occ"] != 0 for d in wrapped) >= 3, [d["occ"] for d in wrapped]
    assert len(details) - len(live) == 11


def test_factor_and_scale_of_the_reference():
    # (the program checks every (ao, strength) and every (byte, m); here the reference's landmarks)
    ao = np.arange(256)
    assert (ao_ref.ao_factor(ao, 0) == 255).all() and (ao_ref.ao_factor(ao, 255) == ao).all()
    assert int(ao_ref.ao_factor(53, 96)) == 255 - (202 * 96 + 127) // 255 == 179
    assert int(ao_ref.scale_rgb(0xAB123456, 255)) == 0x123456 and int(ao_ref.scale_rgb(0xFFFFFF, 128)) == 0x808080
    assert int(ao_ref.scale_rgb(0x010203, 127)) == 0x000101 and int(ao_ref.scale_rgb(0xFFFFFFFF, 0)) == 0
    assert ao_ref.scale_rgb(np.array([0x3F3F3F, 0x101010], np.uint32), np.array([128, 255])).tolist() == [0x202020, 0x101010]


def test_malformed_arguments_are_refused():
    assert subprocess.run([EXE, "--records", "00"], capture_output=True, timeout=60).returncode == 2
    assert subprocess.run([EXE, "--records", "zz" * 64, "00"], capture_output=True, timeout=60).returncode == 2
    assert subprocess.run([EXE, "--records", "00" * 63, "00"], capture_output=True, timeout=60).returncode == 2
