"""Directed inputs for the learned orders' kernels (tests/test_gpu_order_model.py, and on the CPU
tests/test_order_model.py): frames around the lane block's edges with walk-length patterns for
perm_kernel, grids with cost patterns for order_kernel.  Pure numpy: no GPU, no libvr."""
from __future__ import annotations

import numpy as np


def frames(X: int, Y: int):
    """(LW, rows) for a lane block of X x Y pixels: one full block; three block columns, two
    full block rows and a cut one; cut at the right; one pixel past the block both ways
    (padding pixels in both directions); nothing but a cut block, twice."""
    return [(X, Y), (3 * X, 2 * Y + 8), (X + 8, Y), (X + 1, Y + 1), (8, 8), (1, 1)]


def _pack(p, s):
    return (np.asarray(p, dtype=np.uint32) << np.uint32(16) | np.asarray(s, dtype=np.uint32)).astype(np.uint32)


def _zero(LW, rows, X, Y, rng):
    return np.zeros((rows, LW), dtype=np.uint32)


def _ones(LW, rows, X, Y, rng):
    return np.full((rows, LW), 0xFFFFFFFF, dtype=np.uint32)


def _equal(LW, rows, X, Y, rng):
    return np.full((rows, LW), 7 << 16 | 3, dtype=np.uint32)


def _rising(LW, rows, X, Y, rng):
    i = np.arange(rows * LW, dtype=np.uint32).reshape(rows, LW)
    return _pack(i, i >> 1)


def _falling(LW, rows, X, Y, rng):
    return _rising(LW, rows, X, Y, rng)[::-1, ::-1].copy()


def _three_values(LW, rows, X, Y, rng):
    return rng.choice(np.array([5 << 16 | 2, 40 << 16, 300], dtype=np.uint32), size=(rows, LW))


def _random(LW, rows, X, Y, rng):
    return rng.integers(0, 1 << 32, size=(rows, LW), dtype=np.uint64).astype(np.uint32)


def _primary_only(LW, rows, X, Y, rng):
    return _random(LW, rows, X, Y, rng) & np.uint32(0xFFFF0000)


def _shadow_only(LW, rows, X, Y, rng):
    return _random(LW, rows, X, Y, rng) & np.uint32(0x0000FFFF)


def _one_heavy(LW, rows, X, Y, rng):
    w = np.zeros((rows, LW), dtype=np.uint32)
    for y0 in range(0, rows, Y):
        for x0 in range(0, LW, X):
            w[rng.integers(y0, min(y0 + Y, rows)), rng.integers(x0, min(x0 + X, LW))] = 1000 << 16 | 500
    return w


def _equal_weight_pairs(LW, rows, X, Y, rng):
    # (8, 0), (8, 7), (0, 8), (7, 8) all weigh 9 -- the rank key cannot tell them apart, the
    # cost word max(p) + max(s) can -- and (9, 0) weighs 10
    pairs = np.array([8 << 16, 8 << 16 | 7, 8, 7 << 16 | 8, 9 << 16], dtype=np.uint32)
    return rng.choice(pairs, size=(rows, LW))


def _saturated(LW, rows, X, Y, rng):
    return rng.choice(np.array([0xFFFF0000, 0x0000FFFF], dtype=np.uint32), size=(rows, LW))


PCOST_PATTERNS = {"zero": _zero, "all-ones": _ones, "equal": _equal, "rising": _rising, "falling": _falling,
                  "three-values": _three_values, "random": _random, "primary-only": _primary_only,
                  "shadow-only": _shadow_only, "one-heavy": _one_heavy, "equal-weight-pairs": _equal_weight_pairs,
                  "saturated-halves": _saturated}


def pcost(pattern: str, LW: int, rows: int, X: int, Y: int):
    """The (rows, LW) uint32 walk lengths of a pattern; the same for the same arguments."""
    rng = np.random.default_rng([sorted(PCOST_PATTERNS).index(pattern), LW, rows])
    return PCOST_PATTERNS[pattern](LW, rows, X, Y, rng)


GRIDS = [(1, 1), (3, 3), (32, 33), (120, 135)]     # (columns, rows); 32x33 = 1056 groups, 120x135 = 1080p

# costs on both sides of order_kernel's class edges (c >> 2); 508 and above are class 0
EDGE_COSTS = [c for k in (1, 2, 63, 64, 126) for c in (4 * k - 1, 4 * k, 4 * k + 1)] + [
    0, 506, 507, 508, 509, 511, 512, 513, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF]


def _c_equal(n, rng):
    return np.full((n, 2), 77, dtype=np.uint32)


def _c_zero(n, rng):
    return np.zeros((n, 2), dtype=np.uint32)


def _c_own_class(n, rng):
    c = (rng.permutation(n) % 128 * 4).astype(np.uint32)
    return np.stack([c, c], axis=1)


def _c_edges(n, rng):
    c = np.array(EDGE_COSTS, dtype=np.uint32)[rng.permutation(n) % len(EDGE_COSTS)]
    return np.stack([c, np.zeros(n, dtype=np.uint32)], axis=1)


def _c_waves_differ(n, rng):
    c = np.stack([rng.integers(0, 600, n), rng.integers(0, 40, n)], axis=1).astype(np.uint32)
    c[1::2] = c[1::2, ::-1]          # the heavy wave alternates between the two
    return c


def _c_random(n, rng):
    return rng.integers(0, 640, size=(n, 2)).astype(np.uint32)


COST_PATTERNS = {"equal": _c_equal, "zero": _c_zero, "own-class": _c_own_class, "class-edges": _c_edges,
                 "waves-differ": _c_waves_differ, "random": _c_random}


def cost(pattern: str, columns: int, rows: int):
    """The (groups, 2) uint32 costs of a pattern; the same for the same arguments."""
    rng = np.random.default_rng([sorted(COST_PATTERNS).index(pattern), columns, rows])
    return COST_PATTERNS[pattern](columns * rows, rng)
