"""CPU reference of vr_occlusion and vr_shade_lights_ao (include/vr.h): voxel ambient
occlusion over a voxel SET and HIT_DTYPE records, in plain Python integers and one numpy float32
subtraction per tangent axis.

  voxel_set             the world voxels of an (n, 3) array as a set of tuples: "stored" is membership
  detail                everything ao(record) goes through: axis, occupancy pattern, corner levels,
                        q_u, q_w, acc, ao and whether the plane cell p itself is stored
  occlusion             ao of every record, uint32
  ao_factor, scale_rgb  the factor a strength makes of ao, and a word scaled by it
  apply_ao              vr_shade_lights_ao's words from vr_shade_lights' terms
  shade_lights_ao_rays  the same from rays, built on tests/lights_ref.py and tests/trace_ref.py

tests/test_ao_check.py holds it to the C++ arithmetic (bin/ao_check), tests/test_ao_ref.py keeps the
golden case from being vacuous, tests/test_gpu_ao.py judges the kernels by it."""
from __future__ import annotations

import numpy as np

from tests import lights_ref, trace_ref

F = np.float32
VOXEL = trace_ref.VOXEL
HIT_DTYPE = trace_ref.HIT_DTYPE
OPEN = 255
AMBIENT, ALL = 0, 1

# (du, dw) of bit j of an occupancy pattern: the 3 x 3 cells row by row, the centre left out
CELLS = ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))
CORNERS = ((-1, -1), (1, -1), (-1, 1), (1, 1))
TANGENTS = ((1, 2), (2, 0), (0, 1))


def wrap32(v: int) -> int:
    """v as a wrapped int32."""
    return ((int(v) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def voxel_set(xyz) -> frozenset:
    return frozenset(map(tuple, np.asarray(xyz, dtype=np.int64).reshape(-1, 3).tolist()))


def axis_of(normal):
    """The axis of a normal with exactly one component +1 or -1 and the others 0, else None."""
    n = [int(c) for c in normal]
    if sorted(abs(c) for c in n) != [0, 0, 1]:
        return None
    return next(i for i in range(3) if n[i] != 0)


def corner_level(s1: int, s2: int, c: int) -> int:
    return 0 if (s1 and s2) else 3 - (s1 + s2 + c)


def q_of(point, voxel: int, region: int) -> int:
    """The position on the face along one axis in 0..256: one float32 subtraction, times 256
    (exact), NaN and everything not above 0 give 0, 256 and more give 256, else truncated."""
    local = wrap32(int(voxel) - 64 * int(region))
    with np.errstate(all="ignore"):
        g = (F(point) - F(np.int32(local))) * F(256.0)
    if not g > 0:
        return 0
    if g >= 256:
        return 256
    return int(g)


def detail(voxels, rec):
    """None for a record that is open by definition (not a VOXEL hit, or no unit axis normal), else
    a dict: axis, occ (the pattern, bit j = CELLS[j]), levels (L per CORNERS entry), qu, qw, acc,
    ao, p_stored."""
    if int(rec["status"]) != VOXEL:
        return None
    a = axis_of(rec["normal"])
    if a is None:
        return None
    u, w = TANGENTS[a]
    p = [wrap32(int(rec["voxel"][i]) + int(rec["normal"][i])) for i in range(3)]

    def stored(du, dw):
        c = list(p)
        c[u], c[w] = wrap32(c[u] + du), wrap32(c[w] + dw)
        return int(tuple(c) in voxels)

    occ = sum(stored(du, dw) << j for j, (du, dw) in enumerate(CELLS))
    levels = [corner_level(stored(su, 0), stored(0, sw), stored(su, sw)) for su, sw in CORNERS]
    qu = q_of(rec["point"][u], rec["voxel"][u], rec["region"][u])
    qw = q_of(rec["point"][w], rec["voxel"][w], rec["region"][w])
    acc = ((256 - qu) * (256 - qw) * levels[0] + qu * (256 - qw) * levels[1] + (256 - qu) * qw * levels[2]
           + qu * qw * levels[3])
    return {"axis": a, "occ": occ, "levels": levels, "qu": qu, "qw": qw, "acc": acc,
            "ao": (acc * 255 + 98304) // 196608, "p_stored": tuple(p) in voxels}


def occlusion(voxels, recs) -> np.ndarray:
    """ao of every record of a HIT_DTYPE array."""
    out = np.full(len(recs), OPEN, dtype=np.uint32)
    for i, rec in enumerate(recs):
        d = detail(voxels, rec)
        if d is not None:
            out[i] = d["ao"]
    return out


def ao_factor(ao, strength: int):
    ao = np.asarray(ao, dtype=np.int64)
    return 255 - ((255 - ao) * int(strength) + 127) // 255


def scale_rgb(words, m):
    """Each of the bytes R, G, B of the words replaced by (b * m + 127) // 255; bits 24-31 dropped."""
    words, m = np.asarray(words, dtype=np.uint32).astype(np.int64), np.asarray(m, dtype=np.int64)
    out = np.zeros(np.broadcast(words, m).shape, dtype=np.int64)
    for sh in (16, 8, 0):
        out |= ((((words >> sh) & 0xFF) * m + 127) // 255) << sh
    return out.astype(np.uint32)


def apply_ao(light_terms, ambient_terms, ao, strength: int, apply: int) -> np.ndarray:
    """vr_shade_lights_ao's words: light_terms a list of uint32 arrays (one per light), ambient_terms
    one array or None, ao the occlusion of every ray's hit."""
    m = ao_factor(ao, strength)
    n = len(ao)
    terms = list(light_terms)
    if apply == AMBIENT:
        if ambient_terms is not None:
            terms.append(scale_rgb(ambient_terms, m))
        return lights_ref.combine(terms) if terms else np.zeros(n, dtype=np.uint32)
    assert apply == ALL
    if ambient_terms is not None:
        terms.append(ambient_terms)
    return scale_rgb(lights_ref.combine(terms), m) if terms else np.zeros(n, dtype=np.uint32)


def shade_lights_ao_rays(scene, voxels, lights, rays, scale, longest, strength, apply, translation=(0.0, 0.0, 0.0),
                         ambient=None):
    """(words, ao) vr_shade_lights_ao writes for a RAY_DTYPE array: scene a pyref.Scene, voxels its
    voxel_set."""
    recs, _ = trace_ref.trace_rays(scene, rays, scale, longest, translation)
    ao = occlusion(voxels, recs)
    terms = lights_ref.light_terms(scene, lights, rays, scale, longest, translation)
    amb = None if ambient is None else lights_ref.ambient_terms(scene, ambient, rays, scale, longest, translation)
    return apply_ao(terms, amb, ao, strength, apply), ao
