"""The CPU reference of vr_shade (tests/shade_ref.py) against the C oracle: for the camera rays
(tests/trace_ref.py) of every pixel of the golden 32 x 24 frame, shade_ray is the oracle's
rendered pixel, word for word -- both stores, both algorithms, each lighting of
shade_ref.LIGHTINGS (the default directional light with and without shadows, the direction
makeUnitVector(1, 2, 3), a point light at (40, 90, 30))."""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest

import oracle
from tests import pyref, shade_ref, trace_ref
from tests.helpers import GOLDEN

W, H, SCALE = 32, 24, 12
STORES = [oracle.STORE_VCS, oracle.STORE_HASHTABLE]
ALGOS = [oracle.ALGO_ORIGINAL, oracle.ALGO_LONGESTAXIS]


@functools.lru_cache(maxsize=None)
def golden():
    d = np.load(os.path.join(GOLDEN, "c1_scene.npz"))
    i = np.arange(W * H)
    cam = oracle.reference_camera(W, H)
    rays = trace_ref.camera_rays(cam, W, H, (i % W).astype(np.uint32), (i // W).astype(np.uint32))
    return d["xyz"], d["rgb"], cam, rays


@pytest.mark.parametrize("name", list(shade_ref.LIGHTINGS))
@pytest.mark.parametrize("algo", ALGOS, ids={oracle.ALGO_ORIGINAL: "ORIGINAL", oracle.ALGO_LONGESTAXIS: "LONGEST_AXIS"}.get)
@pytest.mark.parametrize("store", STORES, ids={oracle.STORE_VCS: "VCS", oracle.STORE_HASHTABLE: "HASH"}.get)
def test_shade_of_camera_rays_is_the_oracles_frame(store, algo, name):
    xyz, rgb, cam, rays = golden()
    spec = shade_ref.LIGHTINGS[name]
    ref = oracle.Scene(xyz, rgb, store)
    want, _ = ref.render(algo, cam, shade_ref.fill_block(oracle.lighting(), *spec), W, H, SCALE)
    ref.close()
    got, never = shade_ref.shade_rays(pyref.Scene(xyz, rgb, store), shade_ref.pyref_lighting(*spec), rays, SCALE,
                                      algo == oracle.ALGO_LONGESTAXIS)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"{bad.size} of {W * H} pixels differ; first at pixel ({int(bad[0]) % W}, {int(bad[0]) // W}): "
                           f"shade_ref 0x{int(got[bad[0]]):06X} oracle 0x{int(want[bad[0]]):06X}")
    assert not (got[never] != 0).any()
    # the frame is no blank: lit pixels and background both
    assert np.count_nonzero(want) >= 30 and np.count_nonzero(want == 0) >= 100
