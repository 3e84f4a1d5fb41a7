"""Seeded ray sets for the vr_trace tests (tests/test_gpu_trace.py).  Pure numpy.

random_rays: n rays around a voxel set, in world space for a given scale and translation
(scene = (world - translation) * scale).  A quarter of the origins lie inside the voxels'
bounding box, the rest on a sphere of 1.5 box diagonals around its centre; every direction aims
at a random point of the box; a third of the directions are rescaled to a length between 1e-3
and 1e3 (the rest keep the distance to their target, so hardly any is a unit vector); every
eighth ray has one direction component zeroed.

degenerate_rays: the rays no caller should send and the walk must still answer as the reference
does -- zero, NaN and infinite directions and origins, an origin far outside float's integer
range, a direction of 1e-30, an axis-aligned ray."""
from __future__ import annotations

import numpy as np

from tests import trace_ref


def random_rays(xyz, seed, n=256, scale=1, translation=(0.0, 0.0, 0.0)):
    rng = np.random.default_rng(seed)
    lo, hi = xyz.min(axis=0).astype(np.float64), xyz.max(axis=0).astype(np.float64) + 1.0
    centre, diag = (lo + hi) / 2.0, float(np.linalg.norm(hi - lo))
    origin = rng.uniform(lo, hi, size=(n, 3))
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    outside = np.arange(n) % 4 != 0
    origin[outside] = centre + 1.5 * diag * u[outside]
    target = rng.uniform(lo, hi, size=(n, 3))
    d = target - origin
    rescale = np.arange(n) % 3 == 1
    length = 10.0 ** rng.uniform(-3.0, 3.0, size=n)
    d[rescale] *= (length / np.linalg.norm(d, axis=1))[rescale, None]
    zeroed = np.flatnonzero(np.arange(n) % 8 == 5)
    d[zeroed, rng.integers(0, 3, size=len(zeroed))] = 0.0
    tr = np.asarray(translation, dtype=np.float64)
    return trace_ref.rays_of(origin / scale + tr, d)


def degenerate_rays(inside, outside):
    """(names, RAY_DTYPE array): `inside` / `outside` are world points in / out of the scene's frame."""
    nan, inf = float("nan"), float("inf")
    cases = [
        ("zero direction, inside", inside, (0.0, 0.0, 0.0)),
        ("zero direction, outside", outside, (0.0, 0.0, 0.0)),
        ("NaN direction, inside", inside, (nan, nan, nan)),
        ("NaN direction, outside", outside, (nan, 1.0, 0.0)),
        ("NaN origin", (nan, inside[1], inside[2]), (0.0, -1.0, 0.0)),
        ("all-NaN origin", (nan, nan, nan), (1.0, 1.0, 1.0)),
        ("infinite direction, inside", inside, (inf, 0.0, 0.0)),
        ("infinite direction, outside", outside, (-inf, -inf, 1.0)),
        ("infinite origin", (inf, inside[1], inside[2]), (-1.0, 0.0, 0.0)),
        ("minus-infinite origin", (-inf, -inf, -inf), (1.0, 1.0, 1.0)),
        ("origin at -3e9", (-3e9, inside[1], inside[2]), (1.0, 0.0, 0.0)),
        ("origin at -3e9, oblique", (-3e9, -3e9, -3e9), (1.0, 1.0, 1.0)),
        ("direction of 1e-30", outside, tuple(1e-30 * (i - o) for i, o in zip(inside, outside))),
        ("direction of 1e-30, inside", inside, (1e-30, -2e-30, 0.5e-30)),
        ("axis-aligned +x", (outside[0], inside[1], inside[2]), (1.0 if inside[0] > outside[0] else -1.0, 0.0, 0.0)),
        ("axis-aligned -y, inside", inside, (0.0, -1.0, 0.0)),
        ("axis-aligned +z, inside", inside, (0.0, 0.0, 5.0)),
    ]
    rays = trace_ref.rays_of([c[1] for c in cases], [c[2] for c in cases])
    return [c[0] for c in cases], rays
