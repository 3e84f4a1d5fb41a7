"""A numpy model of the learned orders' data (csrc/vr_order.hip, DESIGN §4 "Heaviest tile groups
first", "Heaviest pixels together"): from the per-pixel walk lengths a launch records
(KView::pcost) the lane order and the waves' costs perm_kernel makes of them, and the property
a work order made from those costs must have.  Pure numpy: no GPU, no libvr.

Every shape is an argument (`shape`, a mapping): block_x, block_y (the lane block, pixels),
entry_bytes (of a perm entry), seat (0: a slot's lanes in cost order, 1: in ascending Morton
order of the pixel's column and row in the block), and -- these the library does not report,
SHAPE_DEFAULTS -- group_x, group_y (the tile group, 16x8 pixels) and waves (per tile group, 2:
wave w renders the group's 8x8 tile w).  The tests pass what the library reports
(vr_debug_lane_order's info), so they hold for any VR_LANE_BLOCK* / VR_LANE_SEAT build.

pcost: (rows, LW) uint32, primary << 16 | shadow walk length, each half clamped at 0xFFFF as
march_kernel stores it."""
from __future__ import annotations

import numpy as np

SHAPE_DEFAULTS = {"group_x": 16, "group_y": 8, "waves": 2}
UNSPECIFIED = -1          # lane_order's perm entries of a block cut by the grid's edge
ORDER_CLASSES = 128       # order_kernel's cost classes, 4 iterations each, class 0 the heaviest


def morton(px, py):
    """Bit 2i = bit i of the column, bit 2i + 1 = bit i of the row (low four bits of each);
    a fifth column bit is bit 8, a fifth row bit bit 9."""
    def spread4(v):
        v = (v | v << 2) & 0x33
        return (v | v << 1) & 0x55
    return spread4(px & 15) | spread4(py & 15) << 1 | (px >> 4) << 8 | (py >> 4) << 9


def _shape(shape):
    sh = dict(SHAPE_DEFAULTS)
    sh.update(shape)
    X, Y, gw, gh, waves = sh["block_x"], sh["block_y"], sh["group_x"], sh["group_y"], sh["waves"]
    if gw != 8 * waves or gh != 8:
        raise ValueError("the model knows tile groups of `waves` 8x8 tiles side by side only")
    if X % gw or Y % gh or (X * Y) & (X * Y - 1) or sh["seat"] not in (0, 1):
        raise ValueError(f"bad lane block shape {sh}")
    return sh


def key_shift(shape) -> int:
    """log2 of the block's pixels: perm_kernel's rank keys are weight << shift | pixel."""
    return (shape["block_x"] * shape["block_y"]).bit_length() - 1


def weights(pcost, shift: int):
    """A pixel's rank weight: min(max(p, s) + ((p + s) >> 3), 2**(32 - shift) - 1)."""
    w = np.asarray(pcost, dtype=np.uint64)
    p, s = w >> np.uint64(16), w & np.uint64(0xFFFF)
    return np.minimum(np.maximum(p, s) + ((p + s) >> np.uint64(3)), np.uint64((1 << (32 - shift)) - 1))


def grid(LW: int, rows: int, shape):
    """(gx, gy, nbx, nby): the frame's tile groups and lane blocks per side."""
    sh = _shape(shape)
    gx, gy = -(-LW // sh["group_x"]), -(-rows // sh["group_y"])
    kx, ky = sh["block_x"] // sh["group_x"], sh["block_y"] // sh["group_y"]
    return gx, gy, -(-gx // kx), -(-gy // ky)


def _deal(pcost, LW, rows, shape):
    """-> (perm, cost, writes): writes[i] counts how often cost word i was defined."""
    sh = _shape(shape)
    X, Y, gw, gh, waves = sh["block_x"], sh["block_y"], sh["group_x"], sh["group_y"], sh["waves"]
    pcost = np.asarray(pcost, dtype=np.uint32)
    if pcost.shape != (rows, LW):
        raise ValueError(f"pcost is {pcost.shape}, not (rows, LW) = {(rows, LW)}")
    n, shift = X * Y, key_shift(sh)
    kx, ky = X // gw, Y // gh                          # tile groups per block side
    gx, gy, nbx, nby = grid(LW, rows, sh)
    pad = np.zeros((nby * Y, nbx * X), dtype=np.uint64)   # pixels outside the frame count as 0
    pad[:rows, :LW] = pcost
    perm = np.full((nbx * nby, n), UNSPECIFIED, dtype=np.int32)
    cost = np.zeros(gx * gy * waves, dtype=np.uint32)
    writes = np.zeros(gx * gy * waves, dtype=np.int64)
    t = np.arange(n, dtype=np.uint64)
    code = morton(t.astype(np.int64) % X, t.astype(np.int64) // X)

    def define(col, row, wave, value):
        i = (row * gx + col) * waves + wave
        cost[i] = value
        writes[i] += 1

    for BY in range(nby):
        for BX in range(nbx):
            w = pad[BY * Y:(BY + 1) * Y, BX * X:(BX + 1) * X]
            p, s = w >> np.uint64(16), w & np.uint64(0xFFFF)
            if (BX + 1) * kx > gx or (BY + 1) * ky > gy:
                # cut by the grid's edge: the block's 8x8 tiles that exist, perm unused
                for ty in range(Y // 8):
                    for tx in range(X // 8):
                        col, row = BX * kx + tx // waves, BY * ky + ty
                        if col < gx and row < gy:
                            tp, ts = p[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8], s[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8]
                            define(col, row, tx % waves, int(tp.max()) + int(ts.max()))
                continue
            c = weights(w.reshape(-1), shift)
            ranked = (np.sort(c << np.uint64(shift) | t)[::-1] & np.uint64(n - 1)).astype(np.int64)
            p, s = p.reshape(-1), s.reshape(-1)
            for q in range(n // 64):
                slot = ranked[64 * q:64 * q + 64]          # ranks 64 q .. 64 q + 63, heaviest first
                g = q // waves                             # the block's tile group, row-major
                define(BX * kx + g % kx, BY * ky + g // kx, q % waves, int(p[slot].max()) + int(s[slot].max()))
                if sh["seat"] == 1:
                    slot = slot[np.argsort(code[slot], kind="stable")]
                perm[BY * nbx + BX, 64 * q:64 * q + 64] = slot
    return perm, cost, writes


def cost_writes(pcost, LW: int, rows: int, shape):
    """How often lane_order's rules define each of the gx * gy * waves cost words."""
    return _deal(pcost, LW, rows, shape)[2]


def lane_order(pcost, LW: int, rows: int, shape):
    """-> (perm, cost).  perm: (blocks, block pixels) int32, entry 64 q + i the block pixel
    (row * block_x + column) of lane i of wave slot q; UNSPECIFIED throughout a block cut by
    the grid's edge.  cost: (gy, gx, waves) uint32, max(p) + max(s) over each wave's pixels."""
    perm, cost, writes = _deal(pcost, LW, rows, shape)
    if not np.all(writes == 1):
        i = int(np.flatnonzero(writes != 1)[0])
        raise AssertionError(f"cost word {i} defined {int(writes[i])} times")
    gx, gy, _, _ = grid(LW, rows, shape)
    return perm, cost.reshape(gy, gx, -1)


def cost_class(cost, waves: int = 2):
    """order_kernel's class of each tile group: 127 - min(127, max over its waves >> 2)."""
    c = np.asarray(cost, dtype=np.uint32).reshape(-1, waves).max(axis=1).astype(np.int64)
    return ORDER_CLASSES - 1 - np.minimum(ORDER_CLASSES - 1, c >> 2)


def check_work_order(order, cost, gx: int, gy: int, waves: int = 2) -> None:
    """Raises ValueError naming the first offender unless `order` is a permutation of
    (row << 16 | column) over the gx x gy grid along which the groups' cost classes never
    decrease (heaviest class first; the order within a class is free)."""
    order = np.asarray(order, dtype=np.uint32).reshape(-1)
    cls = cost_class(cost, waves)
    n = gx * gy
    if cls.shape[0] != n:
        raise ValueError(f"{cls.shape[0]} groups of costs for a {gx}x{gy} grid")
    if order.shape[0] > n:
        raise ValueError(f"{order.shape[0]} entries for a {gx}x{gy} grid of {n} groups")
    seen = np.full(n, -1, dtype=np.int64)
    last = -1
    for i, e in enumerate(order.tolist()):
        col, row = e & 0xFFFF, e >> 16
        if col >= gx or row >= gy:
            raise ValueError(f"entry {i} = {e:#010x}: (row {row}, column {col}) is outside the {gx}x{gy} grid")
        g = row * gx + col
        if seen[g] >= 0:
            raise ValueError(f"entry {i} = {e:#010x}: group (row {row}, column {col}) was entry {int(seen[g])} already")
        seen[g] = i
    if order.shape[0] < n or np.any(seen < 0):
        g = int(np.flatnonzero(seen < 0)[0])
        raise ValueError(f"group (row {g // gx}, column {g % gx}) is missing from the order")
    for i, e in enumerate(order.tolist()):
        k = int(cls[(e >> 16) * gx + (e & 0xFFFF)])
        if k < last:
            raise ValueError(f"entry {i} = {e:#010x}: class {k} after class {last} (inversion)")
        last = k
