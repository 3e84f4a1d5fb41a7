"""The cases of vr_bounce_rays and vr_shade_lights_reflect, computed once and shared by
tests/test_reflect_check.py, tests/test_reflect_ref.py and tests/test_gpu_reflect.py: the descent of
tests/lights_cases.py' golden 32 x 24 frame (scale 12, the four lights and the ambient term of
tests/lights_ref.py) per (store, algorithm, mirror test), the made-up records no walk writes, and the
mirror corridor."""
from __future__ import annotations

import functools

import numpy as np

from tests import ao_cases, ao_ref, lights_cases, lights_ref, pyref, reflect_ref, trace_ref

W, H, SCALE = lights_cases.W, lights_cases.H, lights_cases.SCALE
PAIRS = ((0, False), (0, True), (1, False), (1, True))      # (store: 0 the cluster store, 1 the hash table; longest axis)
EVERY, BIT = (0, 0), (1, 1)                                  # mirror tests: every voxel, the material bit 0


@functools.lru_cache(maxsize=None)
def golden_levels(store: int, longest: bool, mirror=EVERY):
    """reflect_ref.descend of the golden frame to depth 4 (read-only by convention)."""
    return tuple(reflect_ref.descend(lights_cases.pyref_scene(store), ao_cases.golden_set(), lights_ref.LIGHTS,
                                     lights_cases.frame_rays(), SCALE, longest, reflect_ref.MAX_BOUNCES, mirror,
                                     ambient=lights_ref.AMBIENT))


def golden_words(store: int, longest: bool, k: int, bounces: int, mirror=EVERY, strength=None, apply=ao_ref.AMBIENT):
    if k == 0:
        bounces = 0
    return reflect_ref.fold(golden_levels(store, longest, mirror), k, bounces, strength, apply)


KEY = 0x00FF7F                                               # a colour the golden scene does not store
KEY_MIRROR = (0xFFFFFF, KEY)


@functools.lru_cache(maxsize=None)
def painted_voxels():
    """The golden scene with every third voxel painted KEY: (xyz, rgb, the painted indices)."""
    xyz, rgb = lights_cases.golden_voxels()
    assert not (rgb == KEY).any()
    which = np.arange(0, len(xyz), 3)
    painted = rgb.copy()
    painted[which] = KEY
    painted.setflags(write=False)
    return xyz, painted, which


@functools.lru_cache(maxsize=None)
def painted_levels(store: int, longest: bool, bounces: int = 2):
    """The descent of the golden frame over painted_voxels, only KEY voxels mirrors."""
    xyz, rgb, _ = painted_voxels()
    return tuple(reflect_ref.descend(pyref.Scene(xyz, rgb, int(store)), ao_cases.golden_set(), lights_ref.LIGHTS,
                                     lights_cases.frame_rays(), SCALE, longest, bounces, KEY_MIRROR, ambient=lights_ref.AMBIENT))


def _bits(x) -> float:
    return np.array([x], dtype=np.uint32).view(np.float32)[0]


@functools.lru_cache(maxsize=None)
def made_up():
    """(rays, records) no walk writes: every status, normals that are none (zero, two components, a
    2), region and voxel at the ends of int32, NaN and infinite points and directions, -0.0
    direction components.  The NaNs are the quiet NaN 0x7FC00000 of either sign, whose bits every
    fp32 unit hands on unchanged."""
    I32 = np.iinfo(np.int32)
    nan, inf = _bits(0x7FC00000), np.float32(np.inf)
    normals = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (0, 0, 0), (1, 1, 0), (0, -1, 1),
               (2, 0, 0), (0, 0, -2), (1, 0, I32.min), (I32.max, 0, 0)]
    regions = [(0, 0, 0), (1, -2, 3), (I32.min, I32.max, -1), (I32.max, I32.min, 7), (-1, -1, -1)]
    points = [(0.0, 0.0, 0.0), (3.5, 63.75, 0.125), (63.999996, 1e-30, 17.3), (nan, 1.0, 2.0), (1.0, -nan, inf),
              (-inf, 5.0, nan), (-0.0, 64.0, -1.5), (1e38, -1e38, 3e-39)]
    dirs = [(0.3, -0.7, 0.2), (-0.0, 0.0, 1.0), (0.0, -0.0, -0.0), (nan, 1.0, -1.0), (inf, -inf, 0.5), (-nan, -2.0, inf),
            (1e-40, -1e-40, 3e38), (5.0, 0.0, 0.0)]
    recs, rays = [], []
    k = 0
    for status in (0, 1, 2, 3, 4, 0xFFFFFFFF, 1, 1):
        for normal in normals:
            for t in range(3):
                rec = np.zeros((), dtype=trace_ref.HIT_DTYPE)
                rec["status"], rec["color"], rec["normal"] = status, (0x123456 + k) & 0xFFFFFF, normal
                rec["region"], rec["point"] = regions[k % len(regions)], points[(k // 2) % len(points)]
                rec["voxel"] = ((I32.min, 5, I32.max), (1, 2, 3))[k % 2]
                ray = np.zeros((), dtype=trace_ref.RAY_DTYPE)
                ray["origin"], ray["direction"] = (1.0 + k, nan, -2.0), dirs[(k // 3) % len(dirs)]
                recs.append(rec)
                rays.append(ray)
                k += 1
    rays, recs = np.array(rays, dtype=trace_ref.RAY_DTYPE), np.array(recs, dtype=trace_ref.HIT_DTYPE)
    rays.setflags(write=False)
    recs.setflags(write=False)
    return rays, recs


MADE_UP_FORMS = ((1, (0.0, 0.0, 0.0)), (1, (-3.5, 4.5, -6.5)), (3, (-3.5, 4.5, -6.5)), (12, (0.1, -0.2, 1e6)))   # (scale, translation)

# ---------------------------------------------------------------- roundings and frames
LATTICE_LIGHTS = (lights_ref.LIGHT_A, lights_ref.LIGHT_D)
LATTICE_BOUNCES = 2


@functools.lru_cache(maxsize=None)
def lattice_levels(form: str, store: int, longest: bool):
    """The descent of tests/lattice_cases.py' lattice rays in a form of its FORMS (scale 3 with a
    translation does not map the world origin back exactly; the scene has negative regions)."""
    from tests import lattice_cases
    scale, tr = lattice_cases.FORMS[form]
    return tuple(reflect_ref.descend(lattice_cases.reference_scene(store), _lattice_set(), LATTICE_LIGHTS,
                                     np.array(lattice_cases.family_rays("lattice", form)), scale, longest, LATTICE_BOUNCES,
                                     EVERY, tr, ambient=lights_ref.AMBIENT))


@functools.lru_cache(maxsize=None)
def _lattice_set():
    from tests import lattice_cases
    return ao_ref.voxel_set(lattice_cases.scene_voxels()[0])


# ---------------------------------------------------------------- the mirror corridor
# Two one-voxel slabs z = 10 and z = 37 over x, y in [0, 64) at scale 1, and 300 rays from between
# them that look up or down, nearly along z: every ray hits a slab at every depth.
CORRIDOR_N = 300
CORRIDOR_EYE = (32.3, 31.7, 24.4)
CORRIDOR_LIGHTS = (lights_ref.LIGHT_A, lights_ref.LIGHT_D)
CORRIDOR_AMBIENT = (0.25, 0.25, 0.25)


@functools.lru_cache(maxsize=None)
def corridor_voxels():
    x, y = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
    xyz = np.concatenate([np.stack([x.ravel(), y.ravel(), np.full(4096, z)], axis=1) for z in (10, 37)]).astype(np.int32)
    rgb = (((xyz[:, 0] * 4) << 16) | ((xyz[:, 1] * 4) << 8) | np.where(xyz[:, 2] == 10, 0xC0, 0x40)).astype(np.uint32)
    xyz.setflags(write=False)
    rgb.setflags(write=False)
    return xyz, rgb


@functools.lru_cache(maxsize=None)
def corridor_rays():
    rng = np.random.default_rng(11)
    d = np.empty((CORRIDOR_N, 3), dtype=np.float32)
    d[:, :2] = rng.uniform(-0.149, 0.149, size=(CORRIDOR_N, 2)).astype(np.float32)
    d[:, 2] = np.where(np.arange(CORRIDOR_N) % 2 == 0, 1.0, -1.0)
    rays = trace_ref.rays_of(np.tile(np.array(CORRIDOR_EYE, dtype=np.float32), (CORRIDOR_N, 1)), d)
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def corridor_levels(store: int, longest: bool):
    xyz, rgb = corridor_voxels()
    return tuple(reflect_ref.descend(pyref.Scene(xyz, rgb, int(store)), ao_ref.voxel_set(xyz), CORRIDOR_LIGHTS,
                                     corridor_rays(), 1, longest, reflect_ref.MAX_BOUNCES, EVERY, ambient=CORRIDOR_AMBIENT))
