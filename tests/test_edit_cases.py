"""CPU test of tests/edit_cases.py: the model of vr_scene_edit and the case splitter do
what their docstrings say, and the from-scratch oracle scene of an edited set has the
initial scene's frame (diameter, min_coord) -- the condition under which vr_scene_edit
promises a byte-identical image (include/vr.h)."""
from __future__ import annotations

import numpy as np
import pytest

import oracle
from tests.edit_cases import VOXEL_REMOVE, apply_edits, regions_of, sort_voxels, split_case
from tests.fuzz_cases import make_case, make_wide_case


def test_apply_edits_is_sequential():
    xyz = np.array([[0, 0, 0], [1, 2, 3], [0, 0, 0]], dtype=np.int32)
    rgb = np.array([5, 6, 7], dtype=np.uint32)                    # the later (0,0,0) wins
    exyz = np.array([[1, 2, 3], [9, 9, 9], [9, 9, 9], [4, 4, 4], [4, 4, 4], [-1, -1, -1], [0, 0, 0]], dtype=np.int32)
    ergb = np.array([VOXEL_REMOVE, 11, VOXEL_REMOVE, VOXEL_REMOVE, 12, VOXEL_REMOVE, 13], dtype=np.uint32)
    got = sort_voxels(*apply_edits(xyz, rgb, exyz, ergb))
    assert got[0].tolist() == [[0, 0, 0], [4, 4, 4]] and got[1].tolist() == [13, 12]
    empty = apply_edits(xyz, rgb, xyz, np.full(3, VOXEL_REMOVE, dtype=np.uint32))
    assert empty[0].shape == (0, 3) and empty[1].shape == (0,)


@pytest.mark.parametrize("seed,wide", [(0, False), (1, True)])
def test_split_case(seed, wide):
    c = make_wide_case(seed) if wide else make_case(seed)
    full = dict(zip(map(tuple, c.xyz.tolist()), c.rgb.tolist()))
    ixyz, irgb, exyz, ergb, pins = split_case(c.xyz, c.rgb, np.random.default_rng(seed))
    init = dict(zip(map(tuple, ixyz.tolist()), irgb.tolist()))
    assert len(init) == len(ixyz) and all(full[k] == v for k, v in init.items())
    # one pin per occupied region, in the initial scene, never removed
    regions = {tuple(r) for r in regions_of(c.xyz).tolist()}
    assert {tuple(r) for r in regions_of(pins).tolist()} == regions and len(pins) == len(regions)
    pinset = set(map(tuple, pins.tolist()))
    assert pinset <= set(init)
    edits = list(zip(map(tuple, exyz.tolist()), ergb.tolist()))
    assert not [e for e in edits if e[1] == VOXEL_REMOVE and e[0] in pinset]
    assert all(v == VOXEL_REMOVE or v < (1 << 24) for _, v in edits)
    # about half of the rest is in the initial scene; the batch inserts the other half
    rest = len(full) - len(pins)
    assert 0.4 * rest <= len(init) - len(pins) <= 0.6 * rest
    others = set(full) - set(init)
    assert others and others <= {k for k, v in edits if v != VOXEL_REMOVE}
    # about a third of the unpinned initial voxels is removed, some are recoloured
    removed_stored = {k for k, v in edits if v == VOXEL_REMOVE and k in init}
    unpinned = len(init) - len(pins)
    assert 0.3 * unpinned <= len(removed_stored) <= 0.37 * unpinned + 2
    assert [k for k, v in edits if v != VOXEL_REMOVE and k in init and v != init[k]]
    # removals of absent coordinates, and one coordinate edited twice in either order
    per_coord = {}
    for k, v in edits:
        per_coord.setdefault(k, []).append(v == VOXEL_REMOVE)
    assert [k for k, vs in per_coord.items() if vs[0] and k not in init]
    kinds = {(vs[0], vs[1], k in init) for k, vs in per_coord.items() if len(vs) == 2}
    assert {(False, True, False), (True, False, False)} <= kinds        # fresh: insert-remove, remove-insert
    assert {(True, False, True), (False, True, True)} <= kinds          # stored ones too
    # every edit lies in an occupied region, and the edited set keeps every region
    assert {tuple(r) for r in regions_of(exyz).tolist()} <= regions
    nxyz, nrgb = apply_edits(ixyz, irgb, exyz, ergb)
    assert {tuple(r) for r in regions_of(nxyz).tolist()} == regions
    a, b = oracle.Scene(ixyz, irgb, 0), oracle.Scene(nxyz, nrgb, 0)
    assert (b.diameter, b.min_coord, b.region_count) == (a.diameter, a.min_coord, a.region_count)
    a.close()
    b.close()
