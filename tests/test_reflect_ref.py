"""CPU tests of tests/reflect_ref.py itself, before tests/test_gpu_reflect.py judges the kernels by
it: its bounce is tests/lattice_cases.bounce_rays' reflected ray (the rays the walks are already
held to the reference on) byte for byte on the golden frame, the golden case is not vacuous at any
depth, and without reflectivity or depth it reduces to tests/ao_ref.py and tests/lights_ref.py."""
from __future__ import annotations

import numpy as np

from tests import ao_cases, ao_ref, lattice_cases, lights_cases, lights_ref, reflect_cases, reflect_ref


def test_bounce_is_lattice_cases_reflected_ray_on_the_golden_frame():
    rays = lights_cases.frame_rays()
    assert not (rays["direction"] == 0).any()          # (a zero component is the only place the two rules can differ)
    for store, longest in reflect_cases.PAIRS:
        recs = ao_cases.frame_records(store, longest)
        for scale, tr in ((lights_cases.SCALE, (0.0, 0.0, 0.0)), (3, lattice_cases.TRANSLATION)):
            theirs, src = lattice_cases.bounce_rays(recs, rays, scale, tr)
            h = len(src) // 3
            assert h >= 550
            mine = reflect_ref.bounce(rays, recs, scale, tr)
            assert mine[src[:h]].tobytes() == theirs[:h].tobytes(), (store, longest, scale)
            rest = np.setdiff1d(np.arange(len(rays)), src[:h])
            w = mine[rest].view(np.uint32).reshape(-1, 8)
            assert (w[:, [0, 1, 2, 4, 5, 6]] == reflect_ref.QUIET_NAN).all() and (w[:, [3, 7]] == 0).all()


def test_the_golden_case_reflects_at_every_depth():
    for store, longest in reflect_cases.PAIRS:
        counts = reflect_ref.alive_counts(reflect_cases.golden_levels(store, longest))
        assert len(counts) == 5 and all(c >= f for c, f in zip(counts, (550, 400, 280, 200))), (store, longest, counts)
        counts = reflect_ref.alive_counts(reflect_cases.golden_levels(store, longest, reflect_cases.BIT))
        assert len(counts) == 5 and all(c >= f for c, f in zip(counts, (300, 100, 40, 15))), (store, longest, counts)
        # a list never grows, and every depth changes words
        for mirror in (reflect_cases.EVERY, reflect_cases.BIT):
            lv = reflect_cases.golden_levels(store, longest, mirror)
            assert all(len(b.idx) == int(a.refl.sum()) and set(b.idx) <= set(a.idx) for a, b in zip(lv, lv[1:]))
            prev = reflect_cases.golden_words(store, longest, 96, 0, mirror)
            for bounces in (1, 2, 3, 4):
                cur = reflect_cases.golden_words(store, longest, 96, bounces, mirror)
                assert np.count_nonzero(cur != prev) >= 5, (store, longest, mirror, bounces)
                prev = cur
            assert np.count_nonzero(reflect_cases.golden_words(store, longest, 255, 4, mirror) != prev) >= 100


def test_without_reflectivity_or_depth_it_is_ao_ref_and_lights_ref():
    store, longest = 0, True
    scene, voxels, rays = lights_cases.pyref_scene(store), ao_cases.golden_set(), lights_cases.frame_rays()[200:328]
    plain = lights_ref.shade_lights_rays(scene, lights_ref.LIGHTS, rays, lights_cases.SCALE, longest, ambient=lights_ref.AMBIENT)
    ao_words, _ = ao_ref.shade_lights_ao_rays(scene, voxels, lights_ref.LIGHTS, rays, lights_cases.SCALE, longest, 96, ao_ref.ALL,
                                              ambient=lights_ref.AMBIENT)
    assert np.count_nonzero(plain != ao_words) >= 1
    for k, bounces in ((0, 3), (200, 0), (0, 0)):
        got, counts, recs = reflect_ref.reflect_rays(scene, voxels, lights_ref.LIGHTS, rays, lights_cases.SCALE, longest, k, bounces,
                                                     ambient=lights_ref.AMBIENT)
        assert np.array_equal(got, plain) and len(counts) == 1
        assert recs.tobytes() == ao_cases.frame_records(store, longest)[200:328].tobytes()
        got, _, _ = reflect_ref.reflect_rays(scene, voxels, lights_ref.LIGHTS, rays, lights_cases.SCALE, longest, k, bounces,
                                             ambient=lights_ref.AMBIENT, strength=96, apply=ao_ref.ALL)
        assert np.array_equal(got, ao_words)
    # with both, the cached golden case is reflect_rays' own answer
    got, counts, _ = reflect_ref.reflect_rays(scene, voxels, lights_ref.LIGHTS, rays, lights_cases.SCALE, longest, 96, 1,
                                              ambient=lights_ref.AMBIENT)
    assert np.array_equal(got, reflect_cases.golden_words(store, longest, 96, 1)[200:328]) and counts[0] >= 50
    assert np.count_nonzero(got != plain) >= 50
