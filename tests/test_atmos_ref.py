"""CPU tests that keep the cases of tests/atmos_cases.py from being vacuous, for the reference alone
(tests/atmos_ref.py over tests/reflect_cases.golden_levels): the golden frame has misses and VOXEL
records in numbers at depth 0, misses above and below the horizon at every deeper depth, hits before
the fog, inside it and past its end, an atmosphere frame that differs from the plain reflect frame,
and flags 0 is reflect_ref.fold."""
from __future__ import annotations

import numpy as np
import pytest

from tests import ao_ref, atmos_cases, atmos_ref, reflect_cases, reflect_ref

ATM = atmos_cases.ATMOSPHERE
SCALE = atmos_cases.SCALE


@pytest.mark.parametrize("store,longest", reflect_cases.PAIRS)
def test_the_golden_case_is_not_vacuous(store, longest):
    lv = reflect_cases.golden_levels(store, longest)
    assert len(lv) == reflect_ref.MAX_BOUNCES + 1
    st0 = lv[0].recs["status"]
    assert np.count_nonzero(st0 == atmos_ref.MISS) >= 170 and np.count_nonzero(st0 == atmos_ref.VOXEL) >= 590
    for j in range(1, 5):
        miss = lv[j].recs["status"] == atmos_ref.MISS
        h = atmos_ref.sky_h(ATM, lv[j].rays)[miss]
        assert np.count_nonzero(miss) >= 50 and (h > 0).any() and (h < 0).any(), (j, int(miss.sum()))
    # the fog at depth 0: hits before fog_start, inside the ramp, past fog_end
    vox = st0 == atmos_ref.VOXEL
    q = atmos_ref.fog_q(ATM, lv[0].rays, lv[0].recs, SCALE)[vox]
    assert np.count_nonzero(q == 0) >= 20 and np.count_nonzero((q > 0) & (q < 256)) >= 20 and np.count_nonzero(q == 256) >= 20
    # the sky at depth 0 is not one colour
    sky0 = atmos_ref.sky(ATM, lv[0].rays)[st0 == atmos_ref.MISS]
    assert len(set(sky0.tolist())) >= 10


@pytest.mark.parametrize("store,longest", reflect_cases.PAIRS)
def test_the_atmosphere_shows_and_flags_0_is_the_plain_fold(store, longest):
    lv = reflect_cases.golden_levels(store, longest)
    for k, bounces in ((255, 4), (96, 1), (96, 0)):
        plain = reflect_ref.fold(lv, k, bounces)
        both = atmos_cases.golden_words(store, longest, atmos_ref.SKY | atmos_ref.FOG, k, bounces)
        sky = atmos_cases.golden_words(store, longest, atmos_ref.SKY, k, bounces)
        fog = atmos_cases.golden_words(store, longest, atmos_ref.FOG, k, bounces)
        assert np.count_nonzero(both != plain) >= 100, (k, bounces)
        # the sky alone: every ray that misses at depth 0 (at least 170) is black in the plain frame and a
        # blend of three colours without a zero byte here
        assert np.count_nonzero(sky != plain) >= 170, (k, bounces)
        # the fog alone: with k < 255 the first hit shows through, and at least 20 first hits lie past fog_end
        # (their words are the fog's colour) and 20 more inside the ramp; with k = 255 only the last depth shows
        assert np.count_nonzero(fog != plain) >= (20 if k < 255 else 1), (k, bounces)
        assert np.count_nonzero(both != sky) >= (20 if k < 255 else 1) and np.count_nonzero(both != fog) >= 170
        assert ((both | sky | fog) >> 24 == 0).all()
        assert np.array_equal(atmos_cases.golden_words(store, longest, 0, k, bounces), plain)
        assert np.array_equal(atmos_ref.fold(lv, None, k, bounces, SCALE), plain)
    # with occlusion, through the same fold
    for strength, apply in ((96, ao_ref.AMBIENT), (255, ao_ref.ALL)):
        assert np.array_equal(atmos_cases.golden_words(store, longest, 0, 96, 2, strength=strength, apply=apply),
                              reflect_ref.fold(lv, 96, 2, strength, apply))
    # a miss at depth 0 shows the sky itself, whatever the depth of the call
    miss = lv[0].recs["status"] == atmos_ref.MISS
    sky = atmos_ref.sky(ATM, lv[0].rays)
    assert np.array_equal(atmos_cases.golden_words(store, longest, atmos_ref.SKY, 255, 4)[miss], sky[miss])
    # a deeper depth's sky shows in the mirror: with k = 255 a ray that misses at depth 1 is that depth's sky
    alive1 = lv[1].idx[lv[1].recs["status"] == atmos_ref.MISS]
    sky1 = atmos_ref.sky(ATM, lv[1].rays)[lv[1].recs["status"] == atmos_ref.MISS]
    assert np.array_equal(atmos_cases.golden_words(store, longest, atmos_ref.SKY, 255, 1)[alive1], sky1)
