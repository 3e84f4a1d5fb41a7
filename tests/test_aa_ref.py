"""tests/aa_ref.py on a CPU: aa_frame reproduces the committed oracle-made resolved frames
(tests/golden/aa_frames.npz), the yardstick -- how much of the golden frame a supersampled render
changes, which a pass-through or a nearest-sample "filter" cannot reach -- and resolve on hand-made
frames that pin the definition's corners: the largest sums, bits 24-31, round half up."""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest

import oracle
from tests import aa_ref
from tests.golden import make_aa_frames
from tests.helpers import GOLDEN

W, H, SCALE = make_aa_frames.W, make_aa_frames.H, make_aa_frames.SCALE
PAIRS = [(s, a) for s in make_aa_frames.STORES for a in make_aa_frames.ALGOS]


@functools.lru_cache(maxsize=None)
def oracle_scene(store: str):
    d = np.load(os.path.join(GOLDEN, "c1_scene.npz"))
    return oracle.Scene(d["xyz"], d["rgb"], make_aa_frames.STORES[store])


@functools.lru_cache(maxsize=None)
def fine(store: str, algo: str, S: int):
    f = aa_ref.fine_frame(oracle_scene(store), make_aa_frames.ALGOS[algo], oracle.reference_camera(W, H),
                          oracle.lighting(), W, H, S, SCALE)
    f.setflags(write=False)
    return f


@pytest.mark.parametrize("store,algo", PAIRS)
def test_aa_frame_reproduces_the_golden_frames(store, algo):
    golden = np.load(os.path.join(GOLDEN, "aa_frames.npz"))
    assert sorted(golden.files) == sorted(make_aa_frames.key(s, a, S) for s, a in PAIRS for S in (2, 4))
    for S in (2, 4):
        want = golden[make_aa_frames.key(store, algo, S)]
        assert want.shape == (H, W) and want.dtype == np.uint32
        got = aa_ref.aa_frame(oracle_scene(store), make_aa_frames.ALGOS[algo], oracle.reference_camera(W, H),
                              oracle.lighting(), W, H, S, SCALE)
        assert np.array_equal(got, want.reshape(-1)), f"S={S}"
        assert np.array_equal(got, aa_ref.resolve(fine(store, algo, S), W, H, S))
        # a row range is the slice of the full frame
        part = aa_ref.aa_frame(oracle_scene(store), make_aa_frames.ALGOS[algo], oracle.reference_camera(W, H),
                               oracle.lighting(), W, H, S, SCALE, rows=(5, 17))
        assert np.array_equal(part, want[5:17].reshape(-1))


# floors below the counts made on a CPU for the four pairs at 32 x 24 (S = 2: 493-495 pixels with
# samples of more than one colour, 522-525 resolved words unlike the one-sample render; S = 4:
# 597-598, 611-613; S = 8: 615-616, 626-628)
FLOORS = {2: 450, 4: 550, 8: 570}


@pytest.mark.parametrize("store,algo", PAIRS)
@pytest.mark.parametrize("S", sorted(FLOORS))
def test_yardstick_supersampling_changes_most_of_the_frame(store, algo, S):
    one = oracle_scene(store).render(make_aa_frames.ALGOS[algo], oracle.reference_camera(W, H), oracle.lighting(), W, H,
                                     SCALE)[0]
    f = fine(store, algo, S)
    mixed = aa_ref.mixed_pixels(f, W, H, S)
    changed = int(np.count_nonzero(aa_ref.resolve(f, W, H, S) != one))
    assert mixed >= FLOORS[S] and changed >= FLOORS[S], (mixed, changed)
    # what the floors rule out: a pass-through (the top left sample of every pixel) keeps a pure
    # sample colour at every pixel, so it differs from the mean wherever the samples are mixed
    nearest = f.reshape(H, S, W, S)[:, 0, :, 0].reshape(-1)
    assert np.count_nonzero(nearest != aa_ref.resolve(f, W, H, S)) >= FLOORS[S]


@pytest.mark.parametrize("S", aa_ref.SAMPLES)
def test_resolve_largest_sums_and_top_bits(S):
    w, h = 5, 3
    full = np.full(S * w * S * h, 0x00FFFFFF, dtype=np.uint32)
    assert (aa_ref.resolve(full, w, h, S) == 0x00FFFFFF).all()       # S = 8: each channel sums to 255 * 64
    assert (aa_ref.resolve(full | np.uint32(0xFF000000), w, h, S) == 0x00FFFFFF).all()
    # bits 24-31 are dropped, whatever they hold: the same words with random top bytes
    rng = np.random.default_rng(S)
    low = rng.integers(0, 1 << 24, size=full.size, dtype=np.uint32)
    top = rng.integers(0, 256, size=full.size, dtype=np.uint32) << 24
    assert np.array_equal(aa_ref.resolve(low | top, w, h, S), aa_ref.resolve(low, w, h, S))
    assert (aa_ref.resolve(low | top, w, h, S) >> 24 == 0).all()
    if S == 1:
        assert np.array_equal(aa_ref.resolve(low | top, w, h, 1), low)
    # against a plain loop over the definition
    fine = (low | top).reshape(S * h, S * w)
    want = np.zeros((h, w), dtype=np.uint32)
    for y in range(h):
        for x in range(w):
            word = 0
            for sh in (16, 8, 0):
                total = sum((int(fine[S * y + j, S * x + i]) >> sh) & 0xFF for j in range(S) for i in range(S))
                word |= ((total + S * S // 2) // (S * S)) << sh
            want[y, x] = word
    assert np.array_equal(aa_ref.resolve(fine, w, h, S), want.reshape(-1))


def test_resolve_rounds_half_up():
    # N = 4: k ones among a pixel's four samples, per channel -- sums 0, 1, 2, 3, 4 -> 0, 0, 1, 1, 1
    for k, want in enumerate((0, 0, 1, 1, 1)):
        block = np.array([0x010101] * k + [0] * (4 - k), dtype=np.uint32)
        for order in (block, block[::-1]):
            assert aa_ref.resolve(order.reshape(2, 2), 1, 1, 2)[0] == want * 0x010101, k
    # a checker of 0 and 1 in one channel at a time: every pixel sums to 2 -> 1 in that channel only
    for sh in (16, 8, 0):
        checker = ((np.add.outer(np.arange(4), np.arange(6)) & 1) << sh).astype(np.uint32)
        assert (aa_ref.resolve(checker, 3, 2, 2) == 1 << sh).all()
    # N = 16 and 64: the sum just below and at half
    for S in (4, 8):
        n = S * S
        for k, want in ((n // 2 - 1, 0), (n // 2, 1), (n - 1, 1)):
            block = np.array([0x000100] * k + [0] * (n - k), dtype=np.uint32)
            assert aa_ref.resolve(block.reshape(S, S), 1, 1, S)[0] == want << 8, (S, k)
    with pytest.raises(ValueError):
        aa_ref.resolve(np.zeros(9, np.uint32), 1, 1, 3)
    with pytest.raises(ValueError):
        aa_ref.resolve(np.zeros(5, np.uint32), 1, 1, 2)
