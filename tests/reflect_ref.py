"""CPU reference of vr_bounce_rays and vr_shade_lights_reflect (include/vr.h): mirror
reflections in numpy, built only from tests/ao_ref.py, tests/lights_ref.py, tests/trace_ref.py and
tests/pyref.py (all left as they are).

  bounce        the bounce ray of every (ray, record) pair: the hit point back in world units in five
                float32 operations, the direction with one sign bit flipped, six quiet NaNs for a
                record that has no bounce
  mix           two words blended by k in 0..255, in integers
  descend       depth by depth: the rays alive, their records, their lighting terms and occlusion
  fold          the words of a call from descend's levels, for any reflectivity, depth and occlusion
  reflect_rays  both: (words, the alive counts per depth, the records of depth 0)

tests/test_reflect_check.py holds bounce and mix to the C++ arithmetic (bin/reflect_check),
tests/test_reflect_ref.py ties bounce to tests/lattice_cases.bounce_rays and keeps the golden case
from being vacuous, tests/test_gpu_reflect.py judges the kernels by it."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests import ao_ref, lights_ref, trace_ref

F = np.float32
VOXEL = trace_ref.VOXEL
HIT_DTYPE = trace_ref.HIT_DTYPE
RAY_DTYPE = trace_ref.RAY_DTYPE
QUIET_NAN = trace_ref.QUIET_NAN
MAX_BOUNCES = 4


def axes_of(recs) -> np.ndarray:
    """The axis of every record's bounce: that of a normal with exactly one component +1 or -1 and
    the others 0 in a VOXEL record, else -1."""
    n = recs["normal"].astype(np.int64)
    unit = (np.abs(n) == 1)
    ok = (recs["status"] == VOXEL) & (unit.sum(axis=1) == 1) & ((n != 0).sum(axis=1) == 1)
    return np.where(ok, unit.argmax(axis=1), -1)


def bounce(rays, recs, scale, translation=(0.0, 0.0, 0.0)) -> np.ndarray:
    """bounce(rays[i], recs[i]) for RAY_DTYPE and HIT_DTYPE arrays of one length, as a RAY_DTYPE array."""
    assert len(rays) == len(recs)
    a = axes_of(recs)
    out = np.zeros(len(rays), dtype=RAY_DTYPE)
    with np.errstate(all="ignore"):
        m = (recs["region"].astype(F) * F(64.0)).astype(F)
        s = (m + recs["point"]).astype(F)
        q = (s / F(np.uint32(scale))).astype(F)
        o = (np.asarray(translation, dtype=F) + q).astype(F)
    d = np.ascontiguousarray(rays["direction"]).view(np.uint32).copy()
    flip = a[:, None] == np.arange(3)[None, :]
    d[flip] ^= np.uint32(0x80000000)
    none = a < 0
    ob = np.ascontiguousarray(o).view(np.uint32).copy()
    ob[none] = QUIET_NAN
    d[none] = QUIET_NAN
    out["origin"] = ob.view(F)
    out["direction"] = d.view(F)
    return out


def mix(a, b, k: int) -> np.ndarray:
    """Each of the bytes R, G, B is (A * (255 - k) + B * k + 127) // 255; bits 24-31 are dropped."""
    a, b, k = np.asarray(a, dtype=np.uint32).astype(np.int64), np.asarray(b, dtype=np.uint32).astype(np.int64), int(k)
    out = np.zeros(np.broadcast(a, b).shape, dtype=np.int64)
    for sh in (16, 8, 0):
        out |= ((((a >> sh) & 0xFF) * (255 - k) + ((b >> sh) & 0xFF) * k + 127) // 255) << sh
    return out.astype(np.uint32)


@dataclass
class Level:
    """One depth of a descent: the rays alive at it (their numbers in the call, ascending), their
    rays, records, terms per light, ambient terms (or None) and occlusion, and which of them reflect."""
    idx: np.ndarray
    rays: np.ndarray
    recs: np.ndarray
    terms: list
    amb: np.ndarray | None
    ao: np.ndarray
    refl: np.ndarray


def descend(scene, voxels, lights, rays, scale, longest, bounces, mirror=(0, 0), translation=(0.0, 0.0, 0.0),
            ambient=None) -> list:
    """The levels 0..bounces of a descent (fewer when no ray is left): scene a pyref.Scene, voxels
    its ao_ref.voxel_set.  A ray is alive at depth j + 1 when it is alive at depth j, its record there
    is a VOXEL hit and (color & mask) == value."""
    mask, value = int(mirror[0]), int(mirror[1])
    idx, cur, levels = np.arange(len(rays)), np.array(rays, dtype=RAY_DTYPE), []
    for j in range(int(bounces) + 1):
        recs, _ = trace_ref.trace_rays(scene, cur, scale, longest, translation)
        terms = lights_ref.light_terms(scene, lights, cur, scale, longest, translation)
        amb = None if ambient is None else lights_ref.ambient_terms(scene, ambient, cur, scale, longest, translation)
        refl = (recs["status"] == VOXEL) & ((recs["color"] & np.uint32(mask)) == np.uint32(value))
        levels.append(Level(idx, cur, recs, terms, amb, ao_ref.occlusion(voxels, recs), refl))
        if j == bounces or not refl.any():
            break
        idx, cur = idx[refl], bounce(cur, recs, scale, translation)[refl]
    return levels


def level_words(level: Level, strength=None, apply=ao_ref.AMBIENT) -> np.ndarray:
    """W of a level's rays: vr_shade_lights' words for strength None, vr_shade_lights_ao's otherwise."""
    if strength is None:
        terms = list(level.terms) + ([level.amb] if level.amb is not None else [])
        return lights_ref.combine(terms) if terms else np.zeros(len(level.idx), dtype=np.uint32)
    return ao_ref.apply_ao(level.terms, level.amb, level.ao, strength, apply)


def fold(levels, k: int, bounces: int, strength=None, apply=ao_ref.AMBIENT) -> np.ndarray:
    """colors of the call from its levels (descend with at least `bounces` bounces): C^B = W^B and
    C^j = refl^j ? mix(W^j, C^(j+1), k) : W^j, folded from the back."""
    levels = levels[: int(bounces) + 1]
    n = len(levels[0].idx)
    deep = None                           # C^(j+1), indexed by ray number
    for j in range(len(levels) - 1, -1, -1):
        lv = levels[j]
        c = np.zeros(n, dtype=np.uint32)
        c[lv.idx] = level_words(lv, strength, apply)
        if deep is not None:
            r = lv.idx[lv.refl]
            c[r] = mix(c[r], deep[r], k)
        deep = c
    return deep


def alive_counts(levels) -> list:
    """The rays alive at depth 1, 2, ...: the reflecting rays of depth 0, 1, ... (a trailing level
    without reflecting rays, or the deepest one, adds its own count of what would go on)."""
    return [int(lv.refl.sum()) for lv in levels]


def reflect_rays(scene, voxels, lights, rays, scale, longest, k, bounces, mirror=(0, 0), translation=(0.0, 0.0, 0.0),
                 ambient=None, strength=None, apply=ao_ref.AMBIENT):
    """(words, reflecting rays per depth 0.., records of depth 0) of vr_shade_lights_reflect.  With
    k == 0 or bounces == 0 only depth 0 exists."""
    depth = int(bounces) if int(k) else 0
    levels = descend(scene, voxels, lights, rays, scale, longest, depth, mirror, translation, ambient)
    return fold(levels, k, depth, strength, apply), alive_counts(levels), levels[0].recs
