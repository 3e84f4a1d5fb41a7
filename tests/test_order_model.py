"""CPU tests of the learned orders' numpy model (tests/order_model.py): against a deliberately
naive per-pixel Python loop, that its rules define every cost word of every directed frame
exactly once, and that check_work_order rejects what is not a heaviest-first permutation."""
from __future__ import annotations

import numpy as np
import pytest

from tests import order_cases, order_model

SHAPES = [{"block_x": 16, "block_y": 32, "entry_bytes": 2, "seat": 0},
          {"block_x": 16, "block_y": 16, "entry_bytes": 1, "seat": 1},
          {"block_x": 32, "block_y": 32, "entry_bytes": 2, "seat": 1},
          {"block_x": 32, "block_y": 16, "entry_bytes": 2, "seat": 0}]
SHAPE_IDS = [f"{s['block_x']}x{s['block_y']}-seat{s['seat']}" for s in SHAPES]


def naive(pcost, LW, rows, shape):
    """The same rules, pixel by pixel in plain Python: -> ({(block, entry): pixel} of the full
    blocks, {(row, column, wave): [cost, ...]} with every value a rule gave that word)."""
    X, Y, seat = shape["block_x"], shape["block_y"], shape["seat"]
    n = X * Y
    shift = {256: 8, 512: 9, 1024: 10}[n]
    gx, gy = (LW + 15) // 16, (rows + 7) // 8
    kx, ky = X // 16, Y // 8
    nbx, nby = (gx + kx - 1) // kx, (gy + ky - 1) // ky
    perm, cost = {}, {}

    def halves(x, y):
        w = int(pcost[y, x]) if x < LW and y < rows else 0
        return w >> 16, w & 0xFFFF

    for BY in range(nby):
        for BX in range(nbx):
            full = all((BX * kx + i) < gx and (BY * ky + j) < gy for i in range(kx) for j in range(ky))
            if not full:
                for ty in range(Y // 8):
                    for tx in range(X // 8):
                        col, row, wave = BX * kx + tx // 2, BY * ky + ty, tx % 2
                        if col >= gx or row >= gy:
                            continue
                        mp = ms = 0
                        for j in range(8):
                            for i in range(8):
                                p, s = halves(BX * X + 8 * tx + i, BY * Y + 8 * ty + j)
                                mp, ms = max(mp, p), max(ms, s)
                        cost.setdefault((row, col, wave), []).append(mp + ms)
                continue
            keys = []
            for t in range(n):
                p, s = halves(BX * X + t % X, BY * Y + t // X)
                keys.append((min(max(p, s) + ((p + s) >> 3), 2 ** (32 - shift) - 1), t))
            keys.sort(reverse=True)                  # heaviest first; among equals the higher pixel
            for q in range(n // 64):
                slot = [t for _, t in keys[64 * q:64 * q + 64]]
                mp = max(halves(BX * X + t % X, BY * Y + t // X)[0] for t in slot)
                ms = max(halves(BX * X + t % X, BY * Y + t // X)[1] for t in slot)
                g = q // 2
                cost.setdefault((BY * ky + g // kx, BX * kx + g % kx, q % 2), []).append(mp + ms)
                if seat == 1:
                    slot.sort(key=lambda t: int(order_model.morton(t % X, t // X)))
                for i, t in enumerate(slot):
                    perm[(BY * nbx + BX, 64 * q + i)] = t
    return perm, cost


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_model_equals_a_naive_loop(shape):
    """Three small random grids per block shape, with ties (few distinct values), full 16-bit
    halves, and frames that cut blocks at both edges."""
    X, Y = shape["block_x"], shape["block_y"]
    rng = np.random.default_rng(X * 100 + Y + shape["seat"])
    for LW, rows, top in ((2 * X + 5, Y + 9, 4), (X, 2 * Y, 1 << 16), (X + 17, 2 * Y + 3, 300)):
        pcost = (rng.integers(0, top, (rows, LW)).astype(np.uint32) << np.uint32(16)
                 | rng.integers(0, top, (rows, LW)).astype(np.uint32))
        perm, cost = order_model.lane_order(pcost, LW, rows, shape)
        want_perm, want_cost = naive(pcost, LW, rows, shape)
        gy, gx, waves = cost.shape
        assert sorted(want_cost) == [(r, c, w) for r in range(gy) for c in range(gx) for w in range(waves)]
        for (r, c, w), values in want_cost.items():
            assert values == [int(cost[r, c, w])], (LW, rows, r, c, w)
        got_perm = {(int(b), int(e)): int(perm[b, e]) for b, e in zip(*np.nonzero(perm != order_model.UNSPECIFIED))}
        assert got_perm == want_perm, (LW, rows)
        # a block is specified whole or not at all
        assert set(np.count_nonzero(perm != order_model.UNSPECIFIED, axis=1).tolist()) <= {0, X * Y}


def test_weights_formula():
    w = np.array([0, 8 << 16, 8 << 16 | 7, 7 << 16 | 8, 9 << 16, 0xFFFF0000, 0x0000FFFF, 0xFFFFFFFF], dtype=np.uint32)
    assert order_model.weights(w, 9).tolist() == [0, 9, 9, 9, 10, 65535 + 8191, 65535 + 8191, 65535 + 16383]
    # the clamp: the key's weight field is 32 - shift bits
    assert order_model.weights(w, 16).tolist() == [0, 9, 9, 9, 10, 65535, 65535, 65535]


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_every_cost_word_exactly_once(shape):
    """On every directed frame the rules -- full blocks' slots, cut blocks' 8x8 tiles -- define
    each of the gx * gy * 2 cost words once: none twice, none left out."""
    X, Y = shape["block_x"], shape["block_y"]
    for LW, rows in order_cases.frames(X, Y):
        writes = order_model.cost_writes(order_cases.pcost("random", LW, rows, X, Y), LW, rows, shape)
        gx, gy, _, _ = order_model.grid(LW, rows, shape)
        assert writes.shape == (gx * gy * 2,)
        assert np.all(writes == 1), (LW, rows, np.flatnonzero(writes != 1)[:8])


def test_zero_walk_lengths_deal_pixels_descending():
    """All keys' weights equal: the deal is the pixel index descending (seat rule 0)."""
    shape = SHAPES[0]
    perm, cost = order_model.lane_order(np.zeros((32, 16), dtype=np.uint32), 16, 32, shape)
    assert perm[0].tolist() == list(range(511, -1, -1))
    assert not cost.any()


def test_patterns_are_what_they_say():
    X, Y = 16, 32
    for name in order_cases.PCOST_PATTERNS:
        for LW, rows in order_cases.frames(X, Y):
            w = order_cases.pcost(name, LW, rows, X, Y)
            assert w.shape == (rows, LW) and w.dtype == np.uint32, name
            assert np.array_equal(w, order_cases.pcost(name, LW, rows, X, Y)), name
    w = order_cases.pcost("rising", 48, 72, X, Y).reshape(-1)
    assert np.all(np.diff(order_model.weights(w, 9).astype(np.int64)) >= 0) and order_model.weights(w, 9)[-1] > 0
    w = order_cases.pcost("falling", 48, 72, X, Y).reshape(-1)
    assert np.all(np.diff(order_model.weights(w, 9).astype(np.int64)) <= 0)
    assert len(np.unique(order_cases.pcost("three-values", 48, 72, X, Y))) == 3
    assert np.count_nonzero(order_cases.pcost("one-heavy", 48, 72, X, Y)) == 3 * 3
    w = order_cases.pcost("equal-weight-pairs", 48, 72, X, Y)
    assert len(np.unique(w)) == 5 and sorted(set(order_model.weights(w, 9).reshape(-1).tolist())) == [9, 10]
    # 508 and everything above is class 0, 507 is not
    cls = order_model.cost_class(np.array([[c, 0] for c in order_cases.EDGE_COSTS], dtype=np.uint32))
    for c, k in zip(order_cases.EDGE_COSTS, cls.tolist()):
        assert (k == 0) == (c >= 508), (c, k)
        assert k == 127 - min(127, c // 4)
    assert order_cases.cost("own-class", 32, 33).shape == (1056, 2)
    assert len(np.unique(order_model.cost_class(order_cases.cost("own-class", 32, 33)))) == 128
    assert len(np.unique(order_model.cost_class(order_cases.cost("own-class", 3, 3)))) == 9


def _sorted_order(cost, gx, gy):
    cls = order_model.cost_class(cost)
    g = np.argsort(cls, kind="stable")
    return ((g // gx) << 16 | (g % gx)).astype(np.uint32)


def test_check_work_order_accepts_any_order_within_a_class():
    gx, gy = 5, 4
    cost = order_cases.cost("random", gx, gy)
    order = _sorted_order(cost, gx, gy)
    order_model.check_work_order(order, cost, gx, gy)
    cls = order_model.cost_class(cost)[(order >> 16) * gx + (order & 0xFFFF)]
    # reverse every run of equal classes: still heaviest first
    rev = np.concatenate([order[cls == k][::-1] for k in np.unique(cls)])
    order_model.check_work_order(rev, cost, gx, gy)
    equal = order_cases.cost("equal", gx, gy)
    order_model.check_work_order(np.random.default_rng(1).permutation(order), equal, gx, gy)


def test_check_work_order_rejects():
    gx, gy = 5, 4
    cost = np.stack([np.arange(20, dtype=np.uint32) * 4, np.zeros(20, dtype=np.uint32)], axis=1)   # group g: class 127 - g
    good = _sorted_order(cost, gx, gy)
    order_model.check_work_order(good, cost, gx, gy)

    dup = good.copy()
    dup[7] = dup[3]
    with pytest.raises(ValueError, match=r"entry 7 .* was entry 3 already"):
        order_model.check_work_order(dup, cost, gx, gy)

    with pytest.raises(ValueError, match=r"group \(row 0, column 0\) is missing"):
        order_model.check_work_order(good[:-1], cost, gx, gy)      # the lightest group, (0, 0), dropped

    for bad in (2 << 16 | 5, 4 << 16 | 1, 0xFFFFFFFF):             # column 5, row 4, an unwritten word
        out = good.copy()
        out[11] = bad
        with pytest.raises(ValueError, match=r"entry 11 .* outside the 5x4 grid"):
            order_model.check_work_order(out, cost, gx, gy)

    inv = good.copy()
    inv[[4, 5]] = inv[[5, 4]]
    with pytest.raises(ValueError, match=r"entry 5 .* class 112 after class 113 \(inversion\)"):
        order_model.check_work_order(inv, cost, gx, gy)

    # the max of a group's two waves decides its class: the same order under swapped costs
    order_model.check_work_order(good, cost[:, ::-1], gx, gy)
    with pytest.raises(ValueError, match="inversion"):
        order_model.check_work_order(good[::-1], cost, gx, gy)
    with pytest.raises(ValueError, match="entries for a"):
        order_model.check_work_order(np.concatenate([good, good[:1]]), cost, gx, gy)
