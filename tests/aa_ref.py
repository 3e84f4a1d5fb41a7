"""CPU reference of vr_resolve and vr_render_aa (include/vr.h): supersampled frames.

  resolve   the box filter in numpy integers.  Pixel (x, y) of the resolved W x H frame has, per
            channel c (R = bits 16-23, G = 8-15, B = 0-7 of a word; bits 24-31 are dropped),
            (sum over the S x S fine words at rows S*y .. S*y+S-1, columns S*x .. S*x+S-1 of c
            + N/2) >> log2(N), N = S * S, packed R << 16 | G << 8 | B.
  aa_frame  resolve of the oracle's own (S * W) x (S * H) render: the fine frame is a render the C
            oracle already makes, so the resolved frame needs no new reference code.

tests/test_aa_ref.py ties both to the committed golden frames (tests/golden/aa_frames.npz) before
tests/test_gpu_aa.py uses them to judge the kernel."""
from __future__ import annotations

import numpy as np

SAMPLES = (1, 2, 4, 8)


def resolve(fine, W: int, H: int, S: int) -> np.ndarray:
    """-> uint32[H * W]: the resolved words of the fine frame `fine` (S*W x S*H words, row-major)."""
    if S not in SAMPLES:
        raise ValueError("samples must be 1, 2, 4 or 8")
    f = np.ascontiguousarray(fine, dtype=np.uint32).reshape(-1)
    if f.size != S * W * S * H:
        raise ValueError("fine frame has the wrong size")
    f = f.reshape(H, S, W, S).astype(np.uint64)
    n, shift = S * S, 2 * (S.bit_length() - 1)
    out = np.zeros((H, W), dtype=np.uint64)
    for sh in (16, 8, 0):
        total = ((f >> np.uint64(sh)) & np.uint64(0xFF)).sum(axis=(1, 3), dtype=np.uint64)
        out |= ((total + np.uint64(n // 2)) >> np.uint64(shift)) << np.uint64(sh)
    return out.astype(np.uint32).reshape(-1)


def fine_frame(oracle_scene, algo, cam, lit, W: int, H: int, S: int, scale: int, rows=None,
               translation=(0.0, 0.0, 0.0)) -> np.ndarray:
    """The oracle's fine rows behind rows [rows[0], rows[1]) of the W x H frame (default: all)."""
    r0, r1 = (0, H) if rows is None else rows
    return oracle_scene.render(int(algo), cam, lit, S * W, S * H, scale, translation, S * r0, S * r1)[0]


def aa_frame(oracle_scene, algo, cam, lit, W: int, H: int, S: int, scale: int, rows=None,
             translation=(0.0, 0.0, 0.0)) -> np.ndarray:
    """-> uint32[rows * W]: rows [rows[0], rows[1]) (default: all) of the resolved W x H frame."""
    r0, r1 = (0, H) if rows is None else rows
    return resolve(fine_frame(oracle_scene, algo, cam, lit, W, H, S, scale, rows, translation), W, r1 - r0, S)


def mixed_pixels(fine, W: int, H: int, S: int) -> int:
    """How many pixels of the W x H frame hold fine samples of more than one colour."""
    f = np.ascontiguousarray(fine, dtype=np.uint32).reshape(H, S, W, S)
    return int(np.count_nonzero((f.max(axis=(1, 3)) != f.min(axis=(1, 3)))))


def seeded_fine(seed: int, words: int) -> np.ndarray:
    """bin/resolve_check --frame's fine words: word k is the high half of x_k+1, x_0 = seed,
    x_k+1 = x_k * 6364136223846793005 + 1442695040888963407 mod 2^64."""
    out = np.zeros(words, dtype=np.uint32)
    x = int(seed)
    for k in range(words):
        x = (x * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        out[k] = x >> 32
    return out
