"""Directed cluster-skip crawl views for tests/test_gpu_crawl_views.py: tiny frames whose
rays graze cluster planes, so that dozens of pixels crawl -- the position pinned on a plane
8k of an absent cluster, direction component there small and negative, creeping by
RN(EPSILON d) per iteration for 10^5..10^6 iterations.  The flagship C5 camera
makes such walks on one direction family at one scale; these cover the three axes, both
algorithms, shadow walks, a scale with a translation, and a point light.

Scene "points": 400 random voxels in [0, 128)^3.  Scene "slab": a 30 %-dense slab at y = 2
over [0, 128)^2 plus 100 random voxels; its views cast shadow rays along a light direction
with one tiny negative component (the shadow walk follows light_dir with a point light
too: Renderer.cuh's shadow rays never aim at light_pos -- the point light changes the
shading of the pixels those walks leave lit).  Pure numpy: no GPU, no libvr.

The oracle's counts of pixels with a walk of >= 65 536 iterations (original / longest axis;
longest walk), of 1536 pixels: y-plane 48 / 48 (371 871), x-plane 160 / 160 (541 391),
x-plane-from-behind 48 / 48 (325 207), z-plane 96 / 96 (993 060), y-plane-scale2 48 / 48
(371 871); shadow walks: shadow-x 14 / 11 (736 455), shadow-z 9 / 8 (822 497),
shadow-x-point-light 14 / 11."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

W, H = 48, 32
ASPECT = float(np.float32(W) / np.float32(H))
UP = (0.0, 1.0, 0.0)
LONG_WALK = 65536        # iterations: the tile pass's budget, past which a walk is the crawl pass's


def points_scene():
    rng = np.random.default_rng(0xC4A71)
    xyz = rng.integers(0, 128, size=(400, 3)).astype(np.int32)
    return xyz, rng.integers(1, 1 << 24, size=400, dtype=np.uint32)


def slab_scene():
    rng = np.random.default_rng(0x51AB)
    g = np.argwhere(rng.random((128, 128)) < 0.30)
    slab = np.stack([g[:, 0], np.full(len(g), 2), g[:, 1]], axis=1)
    xyz = np.concatenate([slab, rng.integers(0, 128, size=(100, 3))]).astype(np.int32)
    return xyz, rng.integers(1, 1 << 24, size=len(xyz), dtype=np.uint32)


SCENES = {"points": points_scene, "slab": slab_scene}


@dataclass(frozen=True)
class View:
    name: str
    scene: str
    eye: tuple                       # in the scene's voxel units (world = eye / scale + translation)
    look_at: tuple
    fov: float
    scale: int = 1
    translation: tuple = (0.0, 0.0, 0.0)
    light_dir: tuple | None = None   # un-normalised; None: the reference's (1, 1, 1)
    point: bool = False
    light_pos: tuple = (10.0, 10.0, -10.0)
    shadow: bool = False             # the long walks are shadow walks (else primary walks)

    def world(self, p) -> tuple:
        return tuple(float(c) / self.scale + t for c, t in zip(p, self.translation))


_SLAB_CAM = dict(scene="slab", eye=(60.3, 50.2, 20.1), look_at=(64.0, 2.0, 70.0), fov=40.0, shadow=True)

VIEWS = [
    View("y-plane", "points", (20.5, 16.05, 30.25), (120.0, 15.6, 100.0), 6.0),
    View("x-plane", "points", (40.1, 40.3, 10.2), (39.6, 45.0, 120.0), 6.0),
    View("x-plane-from-behind", "points", (64.1, 40.3, 120.2), (63.6, 45.0, 5.0), 6.0),
    View("z-plane", "points", (100.2, 50.1, 40.02), (10.0, 30.0, 39.5), 10.0),
    View("y-plane-scale2", "points", (20.5, 16.05, 30.25), (120.0, 15.6, 100.0), 6.0, scale=2,
         translation=(3.0, 1.0, -2.0)),
    View("shadow-x", light_dir=(-0.004, 0.7, 0.7), **_SLAB_CAM),
    View("shadow-z", light_dir=(0.7, 0.7, -0.003), **_SLAB_CAM),
    View("shadow-x-point-light", light_dir=(-0.004, 0.7, 0.7), point=True, light_pos=(64.0, 60.0, 64.0), **_SLAB_CAM),
]
MIN_LONG_PIXELS = {False: 20, True: 5}      # primary views, shadow views
