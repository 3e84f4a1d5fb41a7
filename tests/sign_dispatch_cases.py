"""Views for the tile pass's per-ray sign dispatch (tests/test_sign_dispatch_cases.py on the CPU,
tests/test_gpu_sign_dispatch.py on the GPU).

The original walk picks the loop specialised for a ray's direction signs once per ray, and the
ray's whole sequence of region walks runs inside that arm; a wave whose lanes hold several sign
patterns runs them one whole walk after the other.  These views put the sign changes inside
single 8 x 8 tiles and make the lanes of each pattern cross different numbers of regions:

  the scene   sparse, [-64, 64)^3: 2 x 2 x 2 regions around the origin, one of them empty (the
              null-region skip then runs inside an arm), so the grid's centre planes are the
              coordinate planes and a direction component changes sign where the image plane
              crosses one
  plus-x      eye on the x axis outside the grid, looking along +x: d.y and d.z change sign in
              the frame's central tiles
  minus-z     the same along -z: d.x and d.y
  *-inside    the same with the eye inside the grid (no entry clip)
  zero-column raw camera fields: an axis-aligned view whose column 23 has d.z exactly 0 (so
              sign pattern bit 2 is clear there as for d.z < 0) and whose rows straddle y = 0

The views look slightly off the axis where needed so that the sign change falls inside a tile
and not between two.  Pure numpy, as tests/edge_cases.py."""
from __future__ import annotations

import numpy as np

from tests.edge_cases import EdgeCase, F

W, H = 48, 72                        # 16 x 32 lane blocks: six whole ones and a cut row of them
EMPTY_REGION = (0, 0, -1)            # region coordinates of the empty one: x, y in [0, 64), z in [-64, 0)


def scene(seed=21, fill=0.004):
    """Random voxels at `fill` in seven of the eight regions of [-64, 64)^3, and a denser 12^3
    clump in each of those (shadow casters); nothing in EMPTY_REGION."""
    rng = np.random.default_rng(seed)
    pts = []
    for rx in (-1, 0):
        for ry in (-1, 0):
            for rz in (-1, 0):
                if (rx, ry, rz) == EMPTY_REGION:
                    continue
                base = np.array([rx, ry, rz]) * 64
                n = int(64 ** 3 * fill)
                pts.append(rng.integers(0, 64, size=(n, 3)) + base)
                g = np.stack(np.meshgrid(*[np.arange(12)] * 3, indexing="ij"), -1).reshape(-1, 3)
                g = g[rng.random(len(g)) < 0.35]
                pts.append(g + base + rng.integers(8, 44, size=3))
    xyz = np.unique(np.concatenate(pts), axis=0).astype(np.int32)
    rgb = rng.integers(1, 1 << 24, size=len(xyz), dtype=np.uint32)
    return xyz, rgb


def empty_box():
    lo = np.array(EMPTY_REGION, dtype=np.float64) * 64.0
    return lo, lo + 64.0


# (name, shadows, light direction): shadows off; an equal-component light of each sign (shadow
# patterns 7 and 0, the one-division walk); unequal lights in two other octants
LIGHTS = [("noshadow", False, None),
          ("eq-pos", True, (1.0, 1.0, 1.0)),
          ("eq-neg", True, (-1.0, -1.0, -1.0)),
          ("oct-pnp", True, (2.0, -1.0, 3.0)),
          ("oct-npn", True, (-1.0, 3.0, -2.0))]


def views():
    """name -> the camera part of an EdgeCase (no scene, default light)."""
    e = np.zeros((0, 3), np.int32), np.zeros(0, np.uint32)
    q = float(F(23.5) / F(W))        # u of column 23 as the ray generation rounds it
    out = [
        EdgeCase("plus-x", "S1", "signs", *e, eye=(-110.0, 0.0, 0.0), look_at=(0.0, 1.5, -2.5), fov=60.0, W=W, H=H),
        EdgeCase("minus-z", "S1", "signs", *e, eye=(0.0, 0.0, 115.0), look_at=(-2.5, 1.5, 0.0), fov=60.0, W=W, H=H),
        EdgeCase("plus-x-inside", "S2", "signs", *e, eye=(-40.0, 0.0, 0.0), look_at=(0.0, 0.6, -1.0), fov=100.0, W=W, H=H),
        EdgeCase("minus-z-inside", "S2", "signs", *e, eye=(0.0, 0.0, 37.5), look_at=(-1.0, 0.6, 0.0), fov=100.0, W=W, H=H),
        # origin, lower_left, horizontal, vertical: ro.z - origin.z = -q + u * 1 is exactly 0 in column 23
        EdgeCase("zero-column", "S3", "signs", *e, raw=((-100.0, 0.25, 0.0), (-99.0, -0.5, -q), (0.0, 0.0, 1.0),
                                                       (0.0, 1.5, 0.0)), W=W, H=H),
    ]
    return {c.name: c for c in out}


VIEWS = views()


def case(view, light):
    """The EdgeCase of a view under one of LIGHTS (by name), with the scene."""
    import dataclasses
    _, shadows, d = next(x for x in LIGHTS if x[0] == light)
    xyz, rgb = scene()
    return dataclasses.replace(VIEWS[view], name=f"{view}/{light}", xyz=xyz, rgb=rgb, shadows=shadows, light_dir=d)
