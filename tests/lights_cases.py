"""The golden-frame case of vr_shade_lights, computed once per (store, algorithm) and shared by
tests/test_lights_ref.py (which ties it to the C oracle) and tests/test_gpu_lights.py (which holds
the kernels to it): the golden scene (tests/golden/c1_scene.npz), the 32 x 24 frame of
Camera.reference at scale 12, the four lights of tests/lights_ref.py and its ambient term."""
from __future__ import annotations

import functools
import os

import numpy as np

import oracle
from tests import lights_ref, pyref, trace_ref
from tests.helpers import GOLDEN

W, H, SCALE = 32, 24, 12


@functools.lru_cache(maxsize=None)
def golden_voxels():
    d = np.load(os.path.join(GOLDEN, "c1_scene.npz"))
    return d["xyz"], d["rgb"]


@functools.lru_cache(maxsize=None)
def frame_rays():
    """The camera rays of the frame's pixels, row-major (tests/trace_ref.py; never modified)."""
    i = np.arange(W * H)
    rays = trace_ref.camera_rays(oracle.reference_camera(W, H), W, H, (i % W).astype(np.uint32), (i // W).astype(np.uint32))
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def pyref_scene(store: int):
    xyz, rgb = golden_voxels()
    return pyref.Scene(xyz, rgb, int(store))


@functools.lru_cache(maxsize=None)
def frame_terms(store: int, longest: bool):
    """lights_ref's terms of the frame's rays: (one uint32 array per light of lights_ref.LIGHTS, the
    ambient terms under lights_ref.AMBIENT), read-only."""
    sc = pyref_scene(store)
    terms = lights_ref.light_terms(sc, lights_ref.LIGHTS, frame_rays(), SCALE, longest)
    amb = lights_ref.ambient_terms(sc, lights_ref.AMBIENT, frame_rays(), SCALE, longest)
    for a in terms + [amb]:
        a.setflags(write=False)
    return tuple(terms), amb
