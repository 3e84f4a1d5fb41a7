"""CPU tests of the voxel-access models (tests/access_cases.py) against the edit model
(tests/edit_cases.py apply_edits): a paint of stored voxels is the same edits, a paint of absent
voxels is the identity, a lookup is the set's own colours, and the query generator yields what
it promises."""
from __future__ import annotations

import numpy as np
import pytest

from tests.access_cases import (EDGE_VALUES, INT32_MAX, INT32_MIN, VOXEL_ABSENT, absent_in_box, frame_of,
                                lookup_model, paint_model, queries)
from tests.edit_cases import VOXEL_REMOVE, apply_edits, sort_voxels
from tests.fuzz_cases import make_case, make_wide_case

CASES = [("case", 0), ("case", 5), ("wide", 1)]


def voxels(kind, seed):
    c = make_wide_case(seed) if kind == "wide" else make_case(seed)
    return apply_edits(c.xyz[:0], c.rgb[:0], c.xyz, c.rgb)          # (the set, duplicates resolved)


def same_set(a, b):
    ax, ac = sort_voxels(*a)
    bx, bc = sort_voxels(*b)
    return np.array_equal(ax, bx) and np.array_equal(ac, bc)


def test_absent_is_remove():
    assert VOXEL_ABSENT == VOXEL_REMOVE == 0xFFFFFFFF


@pytest.mark.parametrize("kind,seed", CASES)
def test_paint_of_stored_voxels_is_the_same_edits(kind, seed):
    xyz, rgb = voxels(kind, seed)
    rng = np.random.default_rng(seed)
    pick = rng.permutation(len(xyz))[: max(3, len(xyz) // 4)]
    pick = np.concatenate([pick, pick[:3], pick[:3]])               # three coordinates three times each
    ergb = rng.integers(0, 1 << 24, size=len(pick), dtype=np.uint32)
    pxyz, prgb, n_absent = paint_model(xyz, rgb, xyz[pick], ergb)
    assert n_absent == 0
    assert same_set((pxyz, prgb), apply_edits(xyz, rgb, xyz[pick], ergb))
    assert np.array_equal(pxyz, xyz)                                # same coordinates, same order
    for k in range(3):                                              # the last of the three wins
        assert prgb[pick[k]] == ergb[len(ergb) - 3 + k]


@pytest.mark.parametrize("kind,seed", CASES)
def test_paint_of_absent_voxels_is_the_identity(kind, seed):
    xyz, rgb = voxels(kind, seed)
    rng = np.random.default_rng(seed)
    gone = absent_in_box(xyz, 20, rng)
    assert len(gone) == 20
    pxyz, prgb, n_absent = paint_model(xyz, rgb, gone, rng.integers(0, 1 << 24, size=20, dtype=np.uint32))
    assert n_absent == 20 and np.array_equal(pxyz, xyz) and np.array_equal(prgb, rgb)
    # mixed: only the stored half changes anything, and edit restricted to it agrees
    exyz = np.concatenate([gone[:5], xyz[:5], gone[5:10]])
    ergb = rng.integers(0, 1 << 24, size=15, dtype=np.uint32)
    pxyz, prgb, n_absent = paint_model(xyz, rgb, exyz, ergb)
    assert n_absent == 10
    assert same_set((pxyz, prgb), apply_edits(xyz, rgb, exyz[5:10], ergb[5:10]))


@pytest.mark.parametrize("kind,seed", CASES)
def test_lookup_model_and_queries(kind, seed):
    xyz, rgb = voxels(kind, seed)
    assert np.array_equal(lookup_model(xyz, rgb, xyz), rgb)
    q = queries(xyz, np.random.default_rng(seed))
    assert q.dtype == np.int32 and q.shape[1] == 3
    got = lookup_model(xyz, rgb, q)
    have = set(map(tuple, q.tolist()))
    assert set(map(tuple, xyz.tolist())) <= have
    assert np.count_nonzero(got != VOXEL_ABSENT) >= len(xyz)
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    in_box = np.all((q >= lo) & (q <= hi), axis=1)
    assert np.count_nonzero(in_box & (got == VOXEL_ABSENT)) >= len(xyz)
    flo, fhi = frame_of(xyz)
    mid = (flo + fhi) // 2
    for axis in range(3):
        for v in (flo - 1, fhi):
            c = [mid, mid, mid]
            c[axis] = v
            assert tuple(c) in have
    for v in (-1, -64, -65, 63, 64, 65, 7, 8, 9):
        assert v in EDGE_VALUES and (v, v, v) in have
    assert (INT32_MIN, INT32_MIN, INT32_MIN) in have and (INT32_MAX, INT32_MIN, INT32_MAX) in have


def test_the_empty_set():
    xyz, rgb = np.zeros((0, 3), dtype=np.int32), np.zeros(0, dtype=np.uint32)
    q = queries(xyz, np.random.default_rng(0))
    assert len(q) > 0 and np.all(lookup_model(xyz, rgb, q) == VOXEL_ABSENT)
    assert frame_of(xyz) == (0, 64)
    assert paint_model(xyz, rgb, q, np.zeros(len(q), dtype=np.uint32))[2] == len(q)
