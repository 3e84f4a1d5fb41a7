"""CPU test of the trace reference (tests/trace_ref.py): the ray vr_camera_rays makes for a pixel,
walked as vr_trace walks any ray, gives the record the pick reference gives for that pixel --
every pixel of a small frame, both stores, both algorithms.  pick_ref is held to the C oracle
by tests/test_pick_ref.py, so this ties trace_ref to the same yardstick."""
from __future__ import annotations

import os

import numpy as np
import pytest

import oracle
from tests import pick_ref, pyref, trace_ref
from tests.helpers import GOLDEN

PAIRS = [(s, a) for s in (oracle.STORE_VCS, oracle.STORE_HASHTABLE) for a in (oracle.ALGO_ORIGINAL, oracle.ALGO_LONGESTAXIS)]
PAIR_ID = lambda p: f"{'vcs' if p[0] == 0 else 'hash'}-{'original' if p[1] == 1 else 'longest'}"   # noqa: E731


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_ID)
def test_trace_of_camera_ray_is_the_pick(pair):
    store, algo = pair
    d = np.load(os.path.join(GOLDEN, "c1_scene.npz"))
    ps = pyref.Scene(d["xyz"], d["rgb"], store)
    W, H, scale = 32, 24, 12
    cam = pick_ref.cam_fields(oracle.reference_camera(W, H))
    longest = algo == oracle.ALGO_LONGESTAXIS
    statuses = []
    for y in range(H):
        for x in range(W):
            ray = trace_ref.camera_ray(cam, W, H, x, y)
            assert int(ray["reserved0"]) == 0 and int(ray["reserved1"]) == 0
            got, it = trace_ref.trace_ray(ps, ray["origin"], ray["direction"], scale, longest)
            want, wit, _ = pick_ref.pick_pixel(ps, cam, W, H, x, y, scale, longest)
            assert got.tobytes() == want.tobytes() and it == wit, (x, y, got, want)
            statuses.append(int(got["status"]))
    assert statuses.count(trace_ref.VOXEL) > 50 and statuses.count(trace_ref.MISS) > 50


def test_camera_ray_outside_the_frame_is_nan():
    cam = oracle.reference_camera(32, 24)
    for x, y in ((32, 0), (0, 24), (0xFFFFFFFF, 0xFFFFFFFF)):
        r = trace_ref.camera_ray(cam, 32, 24, x, y)
        assert r.tobytes() == (np.array([trace_ref.QUIET_NAN] * 3 + [0], dtype=np.uint32).tobytes()) * 2


def test_direction_length_does_not_matter_beyond_rounding():
    """A ray and the same ray with its direction scaled by a power of two (exact in binary
    floating point) normalise to the same unit vector: the same record."""
    d = np.load(os.path.join(GOLDEN, "c1_scene.npz"))
    ps = pyref.Scene(d["xyz"], d["rgb"], 0)
    cam = pick_ref.cam_fields(oracle.reference_camera(32, 24))
    ray = trace_ref.camera_ray(cam, 32, 24, 16, 12)
    a, _ = trace_ref.trace_ray(ps, ray["origin"], ray["direction"], 12, False)
    b, _ = trace_ref.trace_ray(ps, ray["origin"], ray["direction"] * np.float32(1024.0), 12, False)
    assert int(a["status"]) == trace_ref.VOXEL and a.tobytes() == b.tobytes()
