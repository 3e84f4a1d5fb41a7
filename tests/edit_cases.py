"""Edit batches for the scene-edit tests (tests/test_gpu_edit.py on the GPU,
tests/test_edit_cases.py on the CPU): the model of vr_scene_edit (plain sequential dict
semantics) and a splitter that turns any voxel set into an initial scene plus one batch
that exercises every action -- insert, overwrite, delete, delete of an absent voxel, and
the same coordinate edited twice in both orders.  Pure numpy: no GPU, no libvr."""
from __future__ import annotations

import numpy as np

VOXEL_REMOVE = 0xFFFFFFFF


def _as_arrays(xyz, rgb):
    return (np.ascontiguousarray(xyz, dtype=np.int32).reshape(-1, 3),
            np.ascontiguousarray(rgb, dtype=np.uint32).reshape(-1))


def _to_dict(xyz, rgb) -> dict:
    xyz, rgb = _as_arrays(xyz, rgb)
    return dict(zip(map(tuple, xyz.tolist()), rgb.tolist()))      # later duplicates win


def _from_dict(d: dict):
    xyz = np.array(list(d.keys()), dtype=np.int32).reshape(-1, 3)
    rgb = np.array(list(d.values()), dtype=np.uint32)
    return xyz, rgb


def apply_edits(xyz, rgb, exyz, ergb):
    """The voxel set (xyz, rgb) after the edits, applied one by one in order: a colour sets
    the voxel (insert or overwrite), VOXEL_REMOVE deletes it (absent: nothing happens)."""
    d = _to_dict(xyz, rgb)
    exyz, ergb = _as_arrays(exyz, ergb)
    for c, v in zip(map(tuple, exyz.tolist()), ergb.tolist()):
        if v == VOXEL_REMOVE:
            d.pop(c, None)
        else:
            d[c] = v
    return _from_dict(d)


def sort_voxels(xyz, rgb):
    """The set in lexicographic (x, y, z) order, for comparisons."""
    xyz, rgb = _as_arrays(xyz, rgb)
    o = np.lexsort((xyz[:, 2], xyz[:, 1], xyz[:, 0]))
    return xyz[o], rgb[o]


def regions_of(xyz) -> np.ndarray:
    """floor(c / 64) per axis: the 64^3 region of each voxel (VoxelSceneCPU.cuh:19-21)."""
    return np.floor_divide(np.asarray(xyz, dtype=np.int64), 64)


def split_case(xyz, rgb, rng):
    """(init_xyz, init_rgb, exyz, ergb, pins) from a voxel set.

    One voxel per occupied region is pinned: it is in the initial scene and no edit removes
    it, so every region -- and with them the scene's frame -- survives the batch.  The
    initial scene is the pins plus about half of the other voxels.  The batch inserts the
    other half, removes about a third of the unpinned initial voxels, recolours some of the
    initial voxels, removes coordinates that are absent, and edits four coordinates twice:
    a fresh one inserted then removed, a fresh one removed then inserted, a stored one
    removed then inserted and a stored one inserted (recoloured) then removed.  The first
    edit of each such pair opens the batch and the second closes it; the rest is shuffled
    in between.  pins: the pinned coordinates, int32 [regions, 3]."""
    xyz, rgb = _from_dict(_to_dict(xyz, rgb))
    n = len(xyz)
    reg = regions_of(xyz)
    _, first = np.unique(reg, axis=0, return_index=True)
    pinned = np.zeros(n, dtype=bool)
    pinned[first] = True
    in_init = pinned | (rng.random(n) < 0.5)
    init_xyz, init_rgb = xyz[in_init], rgb[in_init]
    present = set(map(tuple, xyz.tolist()))

    def fresh():
        while True:
            base = reg[first[int(rng.integers(0, len(first)))]] * 64
            c = tuple(int(v) for v in base + rng.integers(0, 64, size=3))
            if c not in present:
                present.add(c)
                return c

    def colour():
        return int(rng.integers(0, 1 << 24))

    unpinned_init = np.flatnonzero(in_init & ~pinned)
    rng.shuffle(unpinned_init)
    k = len(unpinned_init)
    removed = unpinned_init[: k // 3]
    recoloured = np.concatenate([unpinned_init[k // 3: k // 3 + max(1, k // 8)], first[: max(1, len(first) // 2)]])
    twice = unpinned_init[k // 3 + max(1, k // 8):][:2]         # stored, neither removed nor recoloured above

    singles = [(tuple(c), int(v)) for c, v in zip(xyz[~in_init].tolist(), rgb[~in_init].tolist())]
    singles += [(tuple(xyz[i].tolist()), VOXEL_REMOVE) for i in removed]
    singles += [(tuple(xyz[i].tolist()), colour()) for i in recoloured]
    singles += [(fresh(), VOXEL_REMOVE) for _ in range(5)]
    order = rng.permutation(len(singles))
    singles = [singles[i] for i in order]

    a, b = fresh(), fresh()
    head = [(a, colour()), (b, VOXEL_REMOVE)]
    tail = [(a, VOXEL_REMOVE), (b, colour())]
    if len(twice) > 0:
        c = tuple(xyz[twice[0]].tolist())
        head.append((c, VOXEL_REMOVE))
        tail.append((c, colour()))
    if len(twice) > 1:
        d = tuple(xyz[twice[1]].tolist())
        head.append((d, colour()))
        tail.append((d, VOXEL_REMOVE))
    batch = head + singles + tail
    exyz = np.array([c for c, _ in batch], dtype=np.int32).reshape(-1, 3)
    ergb = np.array([v for _, v in batch], dtype=np.uint32)
    return init_xyz, init_rgb, exyz, ergb, xyz[first]
