"""The golden case of vr_occlusion (tests/ao_cases.py: tests/lights_cases.py' 32 x 24 frame of the
golden scene at scale 12, VCS) is no vacuous one: enough hits are occluded, every corner level
occurs, a hit whose plane cell is itself stored exists, the values are many, and the AMBIENT and
ALL frames differ from each other and from the plain vr_shade_lights frame.

Counted with tests/pyref.py, original / longestaxis: 593 / 594 VOXEL hits, 261 / 263 with ao < 255,
101 / 99 distinct values, 4 / 4 hits with a stored plane cell, 14 / 33 / 438 / 1887 corners at
levels 0 / 1 / 2 / 3 (original), the lowest ao 53."""
from __future__ import annotations

import numpy as np
import pytest

import oracle
from tests import ao_cases, ao_ref

VCS = oracle.STORE_VCS


@pytest.mark.parametrize("longest", [False, True], ids=["ORIGINAL", "LONGEST_AXIS"])
def test_golden_frame_floors(longest):
    details = [d for d in ao_cases.frame_details(VCS, longest) if d]
    ao = ao_cases.frame_ao(VCS, longest)
    recs = ao_cases.frame_records(VCS, longest)
    levels = np.bincount([l for d in details for l in d["levels"]], minlength=4)
    counts = {"hits": len(details), "occluded": int(np.count_nonzero(ao < 255)), "distinct": len(set(ao.tolist())),
              "stored p": sum(d["p_stored"] for d in details), "levels": levels.tolist(), "lowest": int(ao.min())}
    print(counts)
    assert len(details) == np.count_nonzero(recs["status"] == ao_ref.VOXEL) >= 500
    assert counts["occluded"] >= 200 and counts["distinct"] >= 50 and counts["stored p"] >= 1
    assert (levels > 0).all(), levels
    assert (ao[recs["status"] != ao_ref.VOXEL] == 255).all() and np.array_equal(ao, ao_ref.occlusion(ao_cases.golden_set(), recs))
    # the frames: plain, AMBIENT and ALL differ pairwise, at full strength and at 96; strength 0 is plain
    plain = ao_cases.frame_words(VCS, longest, None)
    for strength in (255, 96):
        amb = ao_cases.frame_words(VCS, longest, strength, ao_ref.AMBIENT)
        full = ao_cases.frame_words(VCS, longest, strength, ao_ref.ALL)
        diffs = [int(np.count_nonzero(a != b)) for a, b in ((plain, amb), (plain, full), (amb, full))]
        print(strength, diffs)
        assert min(diffs) >= 1, diffs
        # occlusion only darkens, channel by channel, and only where ao < 255
        for frame in (amb, full):
            for sh in (16, 8, 0):
                assert (((frame >> sh) & 0xFF) <= ((plain >> sh) & 0xFF)).all()
            assert (frame[ao == 255] == plain[ao == 255]).all() and not (frame >> 24).any()
    for apply in (ao_ref.AMBIENT, ao_ref.ALL):
        assert np.array_equal(ao_cases.frame_words(VCS, longest, 0, apply), plain)


def test_shade_lights_ao_rays_is_the_frame_case():
    """shade_lights_ao_rays itself, on every seventh ray of the frame."""
    from tests import lights_cases, lights_ref
    rays = lights_cases.frame_rays()[::7]
    sc = lights_cases.pyref_scene(VCS)
    for apply in (ao_ref.AMBIENT, ao_ref.ALL):
        words, ao = ao_ref.shade_lights_ao_rays(sc, ao_cases.golden_set(), lights_ref.LIGHTS, rays, ao_cases.SCALE, False, 96, apply,
                                                ambient=lights_ref.AMBIENT)
        assert np.array_equal(ao, ao_cases.frame_ao(VCS, False)[::7])
        assert np.array_equal(words, ao_cases.frame_words(VCS, False, 96, apply)[::7])
    words, _ = ao_ref.shade_lights_ao_rays(sc, ao_cases.golden_set(), (), rays, ao_cases.SCALE, False, 255, ao_ref.AMBIENT)
    assert not words.any()
