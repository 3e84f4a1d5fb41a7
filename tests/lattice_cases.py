"""Walks that start on the voxel lattice (tests/test_lattice_cases.py on the CPU,
tests/test_gpu_lattice.py on the GPU).

Every other case of the suite starts its walks at points in general position.  These start them
with a coordinate exactly on a voxel face, a cluster plane (a multiple of 8), a region plane (a
multiple of 64) or a face of the scene's frame, and one float32 ulp to either side of such a
plane: `floor` of an exact integer under a negative direction component, the EPSILON nudges from
a plane, entry-clip numerators that are exactly zero.

  SCENE               a half-filled hollow shell two voxels thick over [-20, 84)^3 around a sparse
                      24^3 block at (20, 20, 20): regions -1, 0 and 1 on every axis, so 0 and 64
                      are region planes inside the frame and its faces are at -64 and 128
  lattice_rays        trace rays whose origins have three, two or one coordinate from PLANES (the
                      others fractional), along all 26 directions of {-1, 0, 1}^3 and one oblique
                      direction per sign pattern
  near_lattice_rays   the same rays, one plane coordinate moved one ulp down and one ulp up
  scaled              either family in world units for a scale and a translation; scene_origins
                      is what the walk makes of a world origin, in float32 in the kernel's order:
                      scale 2 with TRANSLATION gives the lattice point back exactly, scale 3 makes
                      near-lattice points of its own
  bounce_rays         rays from the hit points of reference records: reflected, along the normal,
                      and back along the incoming ray
  VIEWS               raw cameras whose image plane is a lattice plane, so that every pixel's
                      origin is a lattice point, in edge_cases.EdgeCase form (cover_run.gpu_camera,
                      gpu_lighting and test_gpu_parity.check_frame take them as they are; the one
                      point light, for which EdgeCase has no field, is written by set_point_light)

Pure numpy: no GPU, no libvr, no oracle."""
from __future__ import annotations

import functools
import itertools
from dataclasses import dataclass

import numpy as np

from tests import pyref, trace_ref
from tests.edge_cases import EdgeCase, block, shell

F = np.float32
W, H = 64, 32                       # four whole 16 x 32 lane blocks; powers of two: (x + 0.5) / W * 64 is exact
TRANSLATION = (-3.5, 4.5, -6.5)     # with scale 2: o / 2 + t and (w - t) * 2 are exact for every lattice o
LO, HI = -20, 84                    # the shell
FRAME_LO, FRAME_HI = -64, 128       # the faces of the scene's frame: regions -1, 0, 1

# what an origin's plane coordinates are drawn from: the frame's faces (-64 inside, 128 outside),
# a point outside the frame on either side (-72, 136), the shell's outer faces (-20, 84), its last
# voxel (83), cluster planes (-8, 8, 32), region planes (0, +-64) and voxel-interior integers (7, 31)
PLANES = (-72.0, -64.0, -20.0, -8.0, 0.0, 7.0, 8.0, 31.0, 32.0, 64.0, 83.0, 84.0, 128.0, 136.0)
AXIS_DIRS = tuple(d for d in itertools.product((-1.0, 0.0, 1.0), repeat=3) if any(d))
OBLIQUE = ((0.3, 0.7, 0.2), (-0.9, 0.1, 0.4), (0.05, -0.8, 0.6), (-0.2, -0.3, 0.9),          # one per sign pattern
           (0.6, 0.25, -0.5), (-0.35, 0.9, -0.15), (0.45, -0.55, -0.7), (-0.65, -0.4, -0.3))
N_RAYS = 624                        # 312 along AXIS_DIRS (12 times each), 312 oblique
ZERO = (0.0, 0.0, 0.0)
FORMS = {"scale1": (1, ZERO), "scale2": (2, TRANSLATION), "scale3": (3, TRANSLATION)}   # name: (scale, translation)
BOUNCE_FORMS = ("scale1", "scale2")


@functools.lru_cache(maxsize=None)
def scene_voxels():
    """(xyz, rgb) of SCENE (read-only arrays: callers share them)."""
    xyz, rgb = shell(21, lo=LO, hi=HI, thick=2, fill=0.5)
    b, c = block(22, (20, 20, 20), size=24, fill=0.3)
    xyz, rgb = np.concatenate([xyz, b]), np.concatenate([rgb, c])
    xyz.setflags(write=False)
    rgb.setflags(write=False)
    return xyz, rgb


@functools.lru_cache(maxsize=None)
def lattice_points(seed=3, n=N_RAYS):
    """-> (origins float32 [n, 3], on_plane bool [n, 3], directions float32 [n, 3]).  Ray k has
    three (k % 3 == 0), one (1) or two (2) coordinates from PLANES; even k take AXIS_DIRS in turn,
    odd k OBLIQUE (3 is coprime to 26 and to 8: every direction meets every kind of origin)."""
    rng = np.random.default_rng(seed)
    o = np.zeros((n, 3), dtype=F)
    on = np.ones((n, 3), dtype=bool)
    d = np.zeros((n, 3), dtype=F)
    for k in range(n):
        o[k] = [PLANES[i] for i in rng.integers(0, len(PLANES), 3)]
        if k % 3 == 1:
            on[k] = np.arange(3) == rng.integers(0, 3)
        elif k % 3 == 2:
            on[k] = np.arange(3) != rng.integers(0, 3)
        for i in np.flatnonzero(~on[k]):
            o[k, i] = F(np.floor(rng.uniform(LO, HI))) + F(rng.uniform(0.0625, 0.9375))
        d[k] = AXIS_DIRS[(k // 2) % 26] if k % 2 == 0 else OBLIQUE[(k // 2) % 8]
    for a in (o, on, d):
        a.setflags(write=False)
    return o, on, d


def lattice_rays(seed=3, n=N_RAYS):
    """RAY_DTYPE array, scene units (scale 1, no translation)."""
    o, _, d = lattice_points(seed, n)
    return trace_ref.rays_of(o, d)


def near_lattice_points(seed=3, n=N_RAYS):
    """-> (origins float32 [2n, 3], moved int [2n], directions): ray 2k is lattice ray k with plane
    coordinate moved[2k] (its plane coordinates in turn, by k) one ulp towards -inf, ray 2k + 1 the
    same one ulp towards +inf.  (From 0 the step is the smallest subnormal.)"""
    o, on, d = lattice_points(seed, n)
    out, moved = np.repeat(o, 2, axis=0), np.zeros(2 * n, dtype=np.int64)
    for k in range(n):
        axes = np.flatnonzero(on[k])
        a = int(axes[k % len(axes)])
        out[2 * k, a] = np.nextafter(o[k, a], F(-np.inf))
        out[2 * k + 1, a] = np.nextafter(o[k, a], F(np.inf))
        moved[2 * k: 2 * k + 2] = a
    return out, moved, np.repeat(d, 2, axis=0)


def near_lattice_rays(seed=3, n=N_RAYS):
    o, _, d = near_lattice_points(seed, n)
    return trace_ref.rays_of(o, d)


def scaled(rays, scale, translation):
    """The rays in world units: origin / scale + translation, in float32 (directions as they are)."""
    out = rays.copy()
    out["origin"] = ((rays["origin"] / F(scale)).astype(F) + np.asarray(translation, dtype=F)).astype(F)
    return out


def scene_origins(rays, scale, translation):
    """Where a walk starts for world rays: (origin - translation) * scale in float32, the
    kernel's (and pyref.Walk.scene's) order of operations."""
    return ((rays["origin"] - np.asarray(translation, dtype=F)).astype(F) * F(scale)).astype(F)


def maps_back(rays, scale, translation):
    """bool [n, 3]: per coordinate, scaled(rays) starts its walk exactly where `rays` does at
    scale 1 (True), or on a float32 beside it (False)."""
    return scene_origins(scaled(rays, scale, translation), scale, translation) == rays["origin"]


def bounce_rays(records, rays, scale=1, translation=(0.0, 0.0, 0.0)):
    """-> (RAY_DTYPE array of 3 h rays, the indices [3 h] of the h VOXEL records they come from).
    The origin is the record's hit point in world units, translation + (region * 64 + point) /
    scale in float32; the directions are the incoming one reflected about the normal, the normal,
    and the incoming one reversed, h rays each in that order."""
    hit = np.flatnonzero(records["status"] == trace_ref.VOXEL)
    r = records[hit]
    o = (np.asarray(translation, dtype=F)
         + ((r["region"].astype(F) * F(64) + r["point"]).astype(F) / F(scale)).astype(F)).astype(F)
    d, n = rays["direction"][hit], r["normal"].astype(F)
    refl = (d - F(2) * (d * n).sum(axis=1, keepdims=True) * n).astype(F)
    return (np.concatenate([trace_ref.rays_of(o, refl), trace_ref.rays_of(o, n), trace_ref.rays_of(o, -d)]),
            np.concatenate([hit, hit, hit]))


FAMILIES = {"lattice": lattice_rays, "near": near_lattice_rays}


@functools.lru_cache(maxsize=None)
def family_rays(family, form):
    """The world rays of a family in a form of FORMS (read-only: callers copy)."""
    scale, tr = FORMS[form]
    rays = scaled(FAMILIES[family](), scale, tr)
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def reference_scene(store):
    return pyref.Scene(*scene_voxels(), int(store))


@functools.lru_cache(maxsize=None)
def reference(family, form, store, longest):
    """(records, iterations) of family_rays(family, form) in the numpy reference, computed once
    per store (0 the cluster store, 1 the hash table) and algorithm."""
    scale, tr = FORMS[form]
    recs, iters = trace_ref.trace_rays(reference_scene(store), family_rays(family, form), scale, bool(longest), tr)
    recs.setflags(write=False)
    iters.setflags(write=False)
    return recs, iters


@functools.lru_cache(maxsize=None)
def bounce_reference(form, store, longest):
    """(bounce rays, the first ray each comes from, records, iterations): bounce_rays of the
    reference's first hits of the lattice rays in `form`, and the reference's records of those."""
    scale, tr = FORMS[form]
    first, _ = reference("lattice", form, store, longest)
    rays, src = bounce_rays(first, family_rays("lattice", form), scale, tr)
    recs, iters = trace_ref.trace_rays(reference_scene(store), rays, scale, bool(longest), tr)
    for a in (rays, src, recs, iters):
        a.setflags(write=False)
    return rays, src, recs, iters


# ---------------------------------------------------------------- views

@dataclass
class LatticeView(EdgeCase):
    """An EdgeCase (raw camera) with what tests/test_lattice_cases.py holds its origins to, and
    an optional point light (world units), which EdgeCase has no field for: set_point_light
    writes it over the struct cover_run.gpu_lighting / test_edge_cases.oracle_lighting made."""
    axis: int = 2                    # the image plane is `axis` = plane, in scene units
    plane: float = 0.0
    first: tuple = (0.0, 0.0)        # pixel (x, y) starts at first + (x, H - y) * step on the other two axes
    step: float = 1.0
    point_light: tuple | None = None


def set_point_light(lit_struct, view):
    """Write the view's point light (if it has one) into a vr_lighting / or_lighting struct."""
    if view.point_light is not None:
        lit_struct.use_point_light = 1
        for i in range(3):
            lit_struct.light_pos[i] = float(view.point_light[i])
    return lit_struct


def plane_view(name, axis, plane, eye, first, scale=1, translation=(0.0, 0.0, 0.0), step=1.0, **kw):
    """A raw camera whose image plane is `axis` = plane (scene units).  Pixel (x, y) starts at
    first + x * step on the plane's first other axis and first + (H - y) * step on its second
    (first: that pair in scene units; H - y runs over 1 .. H), both exact in float32: W, H and the
    steps are powers of two.  At scale s the world fields are the scene's / s + translation."""
    a, b = [i for i in range(3) if i != axis]
    ll, hor, ver = [0.0] * 3, [0.0] * 3, [0.0] * 3
    ll[axis], ll[a], ll[b] = plane, first[0] - 0.5 * step, first[1] - 0.5 * step
    hor[a], ver[b] = W * step, H * step
    world = lambda p: tuple(float(p[i]) / scale + translation[i] for i in range(3))   # noqa: E731
    raw = (world(eye), world(ll), tuple(v / scale for v in hor), tuple(v / scale for v in ver))
    xyz, rgb = scene_voxels()
    return LatticeView(name, "lattice", "lattice", xyz, rgb, raw=raw, scale=scale, translation=translation, W=W, H=H,
                       axis=axis, plane=plane, first=first, step=step, **kw)


def make_views():
    """Inside the shell a light from outside reaches hardly any face (a shadow ray runs to the
    frame's edge, whatever the light), so those views render without shadows; the three that look
    at the shell from outside keep their shadows, with lights on the camera's side."""
    return [
        # an interior integer z, integer eye: the directions (x - 32, y - 32, -32) are integer
        # vectors, through exact voxel corners and edges
        plane_view("z40-integer-eye", 2, 40.0, (32.0, 32.0, 72.0), (0.0, 16.0), shadows=False),
        # the same plane, a fractional eye: one primary walk crawls for 3 x 10^5 iterations
        plane_view("z40-fractional-eye", 2, 40.0, (32.3, 31.7, 72.4), (0.0, 16.0), shadows=False),
        # a cluster plane just under the shell, looking up at its outer face, with a point light
        # on the camera's side and shadows on (the shadow rays of a point light run along the
        # directional light all the same, so that points away from the shell too)
        plane_view("z-24-cluster-plane-point-light", 2, -24.0, (32.0, 32.0, -56.0), (0.0, 16.0), shadows=True,
                   point_light=(10.5, 50.25, -90.75), light_dir=(-1.0, 1.0, -2.0)),
        # a region plane, looking up: floor of an exact 0 under d.z > 0, d.x and d.y of both signs
        plane_view("z0-region-plane", 2, 0.0, (32.0, 32.0, -32.0), (0.0, 16.0), shadows=False,
                   light_dir=(1.0, 2.0, -3.0)),
        # the frame's lower face, looking in at the shell's outer face; the light's x is 0, so the
        # shadow rays leave the lattice hit points along a plane
        plane_view("z-64-frame-lower-face", 2, -64.0, (32.0, 32.0, -128.0), (0.0, 16.0), shadows=True,
                   light_dir=(0.0, -1.0, -2.0)),
        # the frame's upper face is outside the frame: every walk is background after one iteration
        plane_view("z128-frame-upper-face", 2, 128.0, (32.0, 32.0, 160.0), (0.0, 16.0), shadows=True),
        # a region plane on x, looking down x: floor of an exact 64 under d.x < 0
        plane_view("x64-region-plane", 0, 64.0, (96.0, 32.0, 32.0), (16.0, 0.0), shadows=False),
        # the shell's upper face on y from above, looking down, shadows on, the light's z is 0
        plane_view("y84-shell-face", 1, 84.0, (32.0, 116.0, 32.0), (0.0, 16.0), shadows=True,
                   light_dir=(1.0, 2.0, 0.0)),
        # half steps: origins alternate between lattice and half-lattice points
        plane_view("z40-half-step", 2, 40.0, (16.0, 48.0, 72.0), (0.0, 40.0), step=0.5, shadows=False),
        # scale 2 and a translation: the world fields are halves, the walk's origins integers
        plane_view("z8-scale2", 2, 8.0, (32.0, 32.0, -24.0), (0.0, 16.0), scale=2, translation=TRANSLATION,
                   shadows=False, light_dir=(-1.0, -2.0, -3.0)),
    ]


VIEWS = {v.name: v for v in make_views()}
UPPER_FACE = "z128-frame-upper-face"
LONG_CRAWL = "z40-fractional-eye"                       # the cluster store's longest-axis walk: 322 653 iterations
TIED = tuple(n for n in VIEWS if n != LONG_CRAWL)       # whose picks the numpy reference is held to the oracle on


def frame_pixels(w=W, h=H):
    i = np.arange(w * h)
    return (i % w).astype(np.uint32), (i // w).astype(np.uint32)
