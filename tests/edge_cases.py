"""Directed render cases at the guard edges of the walk kernels (tests/test_edge_cases.py on
the CPU, tests/test_gpu_edges.py and tests/cover_run.py on the GPU).

The kernels divide with a hoisted reciprocal (vr::div_fast, vr_device.h) that is proven only
for 2^-64 <= |d| <= 2^20 and 2^-90 <= |n| <= 2^20; outside that domain a lane takes an IEEE
`/` behind a wave ballot.  The random cases of tests/fuzz_cases.py never leave the domain
except through exact zeros, so these cases do, one family per guard:

  E1  a direction component 0 < |d.y| < 2^-64 in part of the frame (mixed waves)
  E2  every ray's d.y tiny, a part of them subnormal
  E3  two tiny direction components (every ray lies on one line: one colour by geometry)
  E4  shadow rays whose light direction has a tiny or subnormal component, on each axis
  E5  entry-clip numerators of 2^20 and more (the far origin comes from scale x translation)
  E6  a non-zero entry-clip numerator below 2^-90
  E7  direction-sign patterns: views from inside a hollow shell that hold every one of the 8
      patterns between them (see sign_cases), tiles that straddle one and two sign-change
      planes, and a pattern-7 view with out-of-domain lanes
  E8  an equal-component light outside the domain (raw vr_lighting fields: the one-division
      shadow walks' fallback, which no unit vector can reach)

A camera is either the reference constructor's arguments (eye, look_at, up, fov) or the raw
vr_camera fields (origin, lower_left, horizontal, vertical): the struct is plain data, and
only raw fields can hold a component that is tiny but not zero.  Pure numpy: no GPU, no libvr,
no oracle."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

F = np.float32
W, H = 48, 32                       # three whole 16 x 32 lane blocks
D_MIN, N_MIN, DOM_MAX = F(2.0 ** -64), F(2.0 ** -90), F(2.0 ** 20)   # div_fast's domain
F32_MIN_NORMAL = F(2.0 ** -126)
E5_FOV = 0.0012                     # degrees: 0.003 lights under 50 pixels, narrowed until >= 200 are lit


@dataclass
class EdgeCase:
    name: str
    family: str
    kind: str                        # which quantity leaves the domain: direction | light | clip | signs
    xyz: np.ndarray
    rgb: np.ndarray
    raw: tuple | None = None         # (origin, lower_left, horizontal, vertical)
    eye: tuple | None = None
    look_at: tuple | None = None
    up: tuple = (0.0, 1.0, 0.0)
    fov: float = 40.0
    scale: int = 1
    translation: tuple = (0.0, 0.0, 0.0)
    shadows: bool = True
    light_dir: tuple | None = None   # un-normalised (makeUnitVector is applied); None: (1, 1, 1)
    raw_light: tuple | None = None   # the struct's light_dir as it stands (no makeUnitVector)
    light_color: tuple = (1.0, 1.0, 1.0)
    stores: tuple = (0, 1)           # 0 the cluster store, 1 the cuckoo hash table
    W: int = W
    H: int = H

    @property
    def aspect(self) -> float:
        return float(F(self.W) / F(self.H))


def block(seed, corner, size=24, fill=0.5):
    """A dense size^3 block at `corner`, each voxel kept with probability `fill`."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(size)] * 3, indexing="ij"), -1).reshape(-1, 3)
    g = g[rng.random(len(g)) < fill] + np.asarray(corner)
    return g.astype(np.int32), rng.integers(1, 1 << 24, size=len(g), dtype=np.uint32)


def shell(seed, lo=4, hi=44, thick=1, fill=0.5):
    """A hollow cube shell [lo, hi)^3 of the given wall thickness."""
    rng = np.random.default_rng(seed)
    n = hi - lo
    g = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3)
    wall = ((g < thick) | (g >= n - thick)).any(axis=1)
    g = g[wall & (rng.random(len(g)) < fill)] + lo
    return g.astype(np.int32), rng.integers(1, 1 << 24, size=len(g), dtype=np.uint32)


def tiny_cases():
    """E1-E3: raw cameras at x = 60 looking along -x at a block that straddles y = 0 and z = 0.
    origin.y and lower_left.y are exactly 0: any other value absorbs v * vy and the component
    becomes an exact zero."""
    xyz, rgb = block(11, (8, -12, -12))
    out = []
    vy = 0.8 * 2.0 ** -63
    out.append(EdgeCase("E1-mixed", "E1", "direction", xyz, rgb, light_dir=(3.0, 1.0, 1.0),
                        raw=((60.0, 0.0, 0.3), (59.0, 0.0, 0.0), (0.0, 0.0, 0.6), (0.0, vy, 0.0))))
    out.append(EdgeCase("E2-subnormal", "E2", "direction", xyz, rgb, light_dir=(3.0, 1.0, -2.0),
                        raw=((60.0, 0.0, 0.3), (59.0, 0.0, 0.0), (0.0, 0.0, 0.6), (0.0, 2.0 ** -124, 0.0))))
    for tag, v in (("2^-63", 2.0 ** -63), ("2^-124", 2.0 ** -124)):
        out.append(EdgeCase(f"E3-two-tiny-{tag}", "E3", "direction", xyz, rgb,
                            light_dir=(8.0, -1.0, 3.0) if v > 1e-30 else (8.0, 1.0, -3.0),
                            raw=((60.0, 0.0, 0.0), (59.0, 0.0, 0.0), (0.0, 0.0, 3.0 * v), (0.0, v, 0.0))))
    return out


def light_cases():
    """E4: an ordinary camera on the lit side, shadows on, the light's tiny (2^-70) or subnormal
    after normalisation (2^-130) component on each axis in turn."""
    xyz, rgb = block(12, (8, 8, 8))
    out = []
    for tag, t in (("2^-70", 2.0 ** -70), ("2^-130", 2.0 ** -130)):
        for axis in range(3):
            d = [1.0, 1.0, 1.0]
            d[axis] = t
            out.append(EdgeCase(f"E4-light-{tag}-{'xyz'[axis]}", "E4", "light", xyz, rgb, eye=(60.0, 45.0, 70.0),
                                look_at=(20.0, 20.0, 20.0), fov=40.0, light_dir=tuple(d)))
    return out


def clip_cases():
    """E5: ray origins at 2^20 and more in scene units, through scale 20000 and a translation 70
    away (an eye that far off in world units would quantise the directions to nothing).  The
    view looks along +x +y +z: EPSILON is absorbed at that magnitude, so only a landing exactly
    on a lower plane of the scene enters it.
    E6: the image plane's x is 2^-100 in every pixel (raw fields: horizontal and vertical have no
    x), so the entry clip's numerator 0 * 64 - o.x is non-zero and below 2^-90; the rays start
    above the scene (y = 90) and the sheared eye sends them down into it."""
    xyz, rgb = block(13, (8, 8, 8))
    e = np.array([0.5, 0.3, 0.2])
    sc = 20000
    tr = e + 70.0
    out = [EdgeCase("E5-far-origin", "E5", "clip", xyz, rgb, eye=tuple(e), look_at=tuple(tr + np.array([20.0] * 3) / sc),
                    fov=E5_FOV, scale=sc, translation=tuple(tr), light_dir=(-1.0, -2.0, -3.0))]
    xyz6, rgb6 = block(14, (8, 8, 8))
    t = 2.0 ** -100
    out.append(EdgeCase("E6-tiny-numerator", "E6", "clip", xyz6, rgb6, light_dir=(-1.0, 2.0, 1.0),
                        raw=((-40.0, 150.0, 20.0), (t, 90.0, 8.0), (0.0, 0.0, 24.0), (0.0, -16.0, 0.0))))
    return out


def sign_cases():
    """E7.  The directions of one camera are eye -> points of a plane that does not hold the
    eye, and such a plane misses the octant opposite its normal: one camera has at most 7 of the
    8 sign patterns.  So two cameras look opposite ways from one eye (non-integer coordinates)
    inside a hollow shell, 150 degrees wide; each holds 7 patterns, together all 8, and tiles
    around the view axis hold up to 7 at once.  The third is E1's camera mirrored to look along
    +x: d.x > 0, d.y tiny and positive, d.z of both signs -- pattern-7 tiles with out-of-domain
    lanes beside pattern-7 tiles without."""
    xyz, rgb = shell(15)
    eye = (24.3, 23.7, 24.6)
    out = [EdgeCase("E7-signs-ppp", "E7", "signs", xyz, rgb, eye=eye, look_at=(25.3, 24.7, 25.6), fov=150.0,
                    light_dir=(1.0, -2.0, -3.0)),
           EdgeCase("E7-signs-nnn", "E7", "signs", xyz, rgb, eye=eye, look_at=(23.3, 22.7, 23.6), fov=150.0,
                    light_dir=(-1.0, -2.0, 3.0))]
    b = block(11, (8, -12, -12))
    out.append(EdgeCase("E7-pattern7-tiny", "E7", "direction", b[0], b[1], light_dir=(-8.0, 2.0, -1.0),
                        raw=((-20.0, 0.0, 0.3), (-19.0, 0.0, 0.0), (0.0, 0.0, 0.6), (0.0, 0.8 * 2.0 ** -63, 0.0))))
    return out


def equal_light_cases():
    """E8: the shadow walks take a one-division loop when the light's components are equal.  A
    unit vector's are then 3^-1/2, inside the domain, so that loop's IEEE fallback is reached only
    by a light that is no unit vector -- vr_lighting is plain data, as vr_camera is: components
    of +-2^-70 each, with a light colour of 2^68 so that the diffuse term 2^68 * 2^-70 still
    lights the pixels.  The camera stands on the lit side for either sign.  The negative light
    is for the hash table only: in the cluster store a skip along such a direction lands exactly
    on its cluster plane (EPSILON * 2^-70 is absorbed), still inside the absent cluster, and the
    reference's shadow walk never finishes -- every pixel 0, which has its own tests."""
    xyz, rgb = block(12, (8, 8, 8))
    t, lc = 2.0 ** -70, (2.0 ** 68,) * 3
    return [EdgeCase("E8-equal-tiny-light-pos", "E8", "light", xyz, rgb, eye=(60.0, 45.0, 70.0), look_at=(20.0, 20.0, 20.0),
                     raw_light=(t, t, t), light_color=lc),
            EdgeCase("E8-equal-tiny-light-neg", "E8", "light", xyz, rgb, eye=(-25.0, -5.0, -30.0),
                     look_at=(20.0, 20.0, 20.0), raw_light=(-t, -t, -t), light_color=lc, stores=(1,))]


def low_face_case():
    """Not a guard's case but the attempt on one argued unreachable (a
    longest-axis jump from a negative cell): a sparse block in the scene's lowest corner, seen
    from above so that every ray leaves through the x = 0, y = 0 or z = 0 face with all three
    direction components negative, through absent clusters (jumps) all the way."""
    xyz, rgb = block(16, (0, 0, 0), size=40, fill=0.02)
    return EdgeCase("low-faces", "attempt", "signs", xyz, rgb, eye=(44.3, 33.1, 51.7), look_at=(-10.0, -5.0, -8.0),
                    fov=22.0, light_dir=(-2.0, -1.0, -3.0))


def all_cases():
    return tiny_cases() + light_cases() + clip_cases() + sign_cases() + equal_light_cases()


CASES = {c.name: c for c in all_cases()}
PAIRS = [(n, s, a) for n, c in CASES.items() for s in c.stores for a in (1, 0)]   # (case, store, 1 original / 0 longest axis)
PICK_CASES = [n for n, c in CASES.items() if c.family in ("E1", "E3", "E5")]


def set_raw(cam_struct, case):
    """Write a raw case's fields into a vr_camera / or_camera struct (forward is not read by a
    render: the image plane's point minus the origin is the direction)."""
    for f, v in zip(("origin", "lower_left", "horizontal", "vertical"), case.raw):
        for i in range(3):
            getattr(cam_struct, f)[i] = float(v[i])
    for i in range(3):
        cam_struct.forward[i] = float(case.raw[1][i]) - float(case.raw[0][i])
    return cam_struct


def fields_of(cam_struct):
    """(origin, lower_left, horizontal, vertical) float32 rows of a camera struct."""
    return np.array([[getattr(cam_struct, f)[i] for i in range(3)]
                     for f in ("origin", "lower_left", "horizontal", "vertical")], dtype=F)


def light(case):
    """The light direction the walks divide by: the raw fields, or makeUnitVector's result."""
    if case.raw_light is not None:
        return np.array(case.raw_light, dtype=F)
    return unit_light(case.light_dir)


def unit_light(light_dir):
    """makeUnitVector in float32: v / sqrt(x x + y y + z z)."""
    d = np.array((1.0, 1.0, 1.0) if light_dir is None else light_dir, dtype=F)
    n = F(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))
    return (d / n).astype(F)


def rays(fields, Wd=W, Ht=H):
    """calculateWorldRay + Camera::generateRay in numpy.float32, operation for operation as the
    kernel's ray generation: -> (ro, rd), float32 [H, W, 3]."""
    org, llc, hor, ver = [np.asarray(f, dtype=F) for f in fields]
    x, y = np.meshgrid(np.arange(Wd), np.arange(Ht))
    u = ((x.astype(F) + F(0.5)) / F(Wd)).astype(F)[..., None]
    v = (((Ht - y).astype(F) + F(0.5)) / F(Ht)).astype(F)[..., None]
    ro = ((llc + u * hor).astype(F) + (v * ver).astype(F)).astype(F)
    c = (ro - org).astype(F)
    with np.errstate(under="ignore"):
        n = np.sqrt(((c[..., 0] * c[..., 0]).astype(F) + (c[..., 1] * c[..., 1]).astype(F)).astype(F)
                    + (c[..., 2] * c[..., 2]).astype(F)).astype(F)
        rd = (c / n[..., None]).astype(F)
    return ro, rd


def divisor_out(d):
    """A divisor outside div_fast's domain but not zero (per component)."""
    a = np.abs(np.asarray(d, dtype=F))
    return (a != 0) & ((a < D_MIN) | (a > DOM_MAX))


def numerator_out(n):
    a = np.abs(np.asarray(n, dtype=F))
    return (a != 0) & ((a < N_MIN) | (a > DOM_MAX))


def clip_numerators(ro, rd, scale, translation, min_coord, diameter):
    """The entry clip's numerators of each ray's first round (rayMarchVoxelScene's clip against
    the scene's planes): (plane * 64) - o with o = scale * (ro - translation), and whether the
    ray starts outside the scene (only then does the clip run)."""
    tr = np.asarray(translation, dtype=F)
    so = (F(scale) * (ro - tr).astype(F)).astype(F)
    lo, hi = int(min_coord), int(min_coord) + int(diameter)
    plane = np.where(rd < 0, F(hi * 64), F(lo * 64)).astype(F)
    cr = np.floor((so / F(64)).astype(F))
    outside = ((cr < lo) | (cr >= hi)).any(axis=-1)
    return (plane - so).astype(F), outside


def sign_pattern(rd):
    """The walk's sign pattern per ray: bit i set when component i is > 0."""
    p = (rd > 0).astype(np.int32)
    return p[..., 0] | (p[..., 1] << 1) | (p[..., 2] << 2)


def tiles(mask_or_values):
    """[H, W] -> [H/8 * W/8, 64]: the 8 x 8 pixel tiles (one wave each, before a lane order)."""
    a = np.asarray(mask_or_values)
    h, w = a.shape
    return a.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)
