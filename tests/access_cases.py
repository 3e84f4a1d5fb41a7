"""Models and queries for the voxel-access tests (tests/test_gpu_access.py on the GPU,
tests/test_access_cases.py on the CPU): vr_scene_lookup is set membership in the scene's voxel
set, vr_scene_paint recolours the stored voxels of a batch with plain sequential dict
semantics, and a generator gives, for any voxel set, the coordinates at which a lookup can go
wrong.  Pure numpy: no GPU, no libvr."""
from __future__ import annotations

import numpy as np

from tests.edit_cases import _as_arrays, _from_dict, _to_dict

VOXEL_ABSENT = 0xFFFFFFFF
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def lookup_model(xyz, rgb, q) -> np.ndarray:
    """uint32[len(q)]: the colour stored at each coordinate of q, or VOXEL_ABSENT."""
    d = _to_dict(xyz, rgb)
    q = np.ascontiguousarray(q, dtype=np.int32).reshape(-1, 3)
    return np.array([d.get(c, VOXEL_ABSENT) for c in map(tuple, q.tolist())], dtype=np.uint32)


def paint_model(xyz, rgb, exyz, ergb):
    """(xyz, rgb, n_absent): the voxel set after the paint, edits applied one by one in order
    (a later edit of a coordinate wins); an edit of a voxel that is not stored does nothing and
    is counted.  The set keeps its coordinates and their order."""
    d = _to_dict(xyz, rgb)
    exyz, ergb = _as_arrays(exyz, ergb)
    n_absent = 0
    for c, v in zip(map(tuple, exyz.tolist()), ergb.tolist()):
        if c in d:
            d[c] = v
        else:
            n_absent += 1
    return (*_from_dict(d), n_absent)


def frame_of(xyz):
    """(lo, hi): the scene's frame in voxels, [lo, hi) per axis -- the 64^3 regions from
    min(0, lowest) to max(0, highest) (VoxelSceneCPU::insertVoxel keeps region 0 inside)."""
    reg = np.floor_divide(np.asarray(xyz, dtype=np.int64).reshape(-1, 3), 64)
    lo = min(0, int(reg.min())) if reg.size else 0
    hi = max(0, int(reg.max())) if reg.size else 0
    return lo * 64, (hi + 1) * 64


def absent_in_box(xyz, count, rng) -> np.ndarray:
    """`count` distinct coordinates of the set's bounding box that are not in the set (all the
    free cells when the box has fewer)."""
    xyz = np.asarray(xyz, dtype=np.int64).reshape(-1, 3)
    if len(xyz) == 0:
        return np.zeros((0, 3), dtype=np.int32)
    lo, hi = xyz.min(axis=0), xyz.max(axis=0) + 1
    stored = set(map(tuple, xyz.tolist()))
    volume = int(np.prod(hi - lo))
    if volume - len(stored) <= 2 * count and volume <= 1 << 22:      # a crowded box: enumerate it
        cells = np.stack(np.meshgrid(*[np.arange(a, b) for a, b in zip(lo, hi)], indexing="ij"), -1).reshape(-1, 3)
        free = np.array([c for c in map(tuple, cells.tolist()) if c not in stored], dtype=np.int64).reshape(-1, 3)
        return free[rng.permutation(len(free))[:count]].astype(np.int32)
    out = set()
    while len(out) < count:
        for c in map(tuple, rng.integers(lo, hi, size=(count, 3)).tolist()):
            if c not in stored and len(out) < count:
                out.add(c)
    return np.array(sorted(out), dtype=np.int32).reshape(-1, 3)


EDGE_VALUES = sorted({m + d for m in list(range(-72, 73, 8)) + [-128, 128, 192] for d in (-1, 0, 1)})


def queries(xyz, rng) -> np.ndarray:
    """int32[n, 3]: every stored voxel; as many absent coordinates of the bounding box; the six
    face-neighbours of the frame (one region outside on each side, touching the frame and a
    region deep); coordinates at +-1 around multiples of 8 and 64 (-1, -64 and -65 among them) on
    each axis beside a stored voxel's other two coordinates, and on the diagonal; and the
    INT32_MIN / INT32_MAX corners, alone and beside a stored voxel's coordinates.  Shuffled."""
    xyz = np.ascontiguousarray(xyz, dtype=np.int32).reshape(-1, 3)
    stored = np.array(list(_to_dict(xyz, np.zeros(len(xyz), dtype=np.uint32)).keys()), dtype=np.int32).reshape(-1, 3)
    parts = [stored, absent_in_box(stored, len(stored), rng)]
    lo, hi = frame_of(stored)
    mid = (lo + hi) // 2
    anchor = [int(v) for v in stored[0]] if len(stored) else [mid, mid, mid]
    extra = []
    for axis in range(3):
        for v in (lo - 1, lo - 64, hi, hi + 63):                      # outside the frame
            c = [mid, mid, mid]
            c[axis] = v
            extra.append(c)
        for v in EDGE_VALUES + [INT32_MIN, INT32_MAX]:
            c = list(anchor)
            c[axis] = v
            extra.append(c)
    extra += [[v, v, v] for v in EDGE_VALUES]
    extra += [[a, b, c] for a in (INT32_MIN, INT32_MAX) for b in (INT32_MIN, INT32_MAX) for c in (INT32_MIN, INT32_MAX)]
    parts.append(np.array(extra, dtype=np.int64).astype(np.int32))
    q = np.concatenate(parts)
    return np.ascontiguousarray(q[rng.permutation(len(q))])
