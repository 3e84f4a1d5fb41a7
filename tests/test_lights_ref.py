"""The CPU reference of vr_shade_lights (tests/lights_ref.py) against the C oracle, on the golden
32 x 24 frame (tests/lights_cases.py): for both stores and both algorithms, the oracle's frames
under each of the four lights, combined, are lights_ref's words of the camera rays -- and the case
is no vacuous one: every light lights its share of the frame, lights overlap, the clamp at 255 is
exercised, and the second light shows pixels the first leaves black."""
from __future__ import annotations

import numpy as np
import pytest

import oracle
from tests import lights_cases, lights_ref

W, H, SCALE = lights_cases.W, lights_cases.H, lights_cases.SCALE
STORES = [oracle.STORE_VCS, oracle.STORE_HASHTABLE]
ALGOS = [oracle.ALGO_ORIGINAL, oracle.ALGO_LONGESTAXIS]

# floors on the frame, counted on the CPU with tests/pyref.py for all four pairs:
# non-zero pixels A 343-347, B 114-123, C 57-62, D 563-567; lit by two or more lights 381-389;
# a channel sum above 255 at 163-177 pixels; black under A but lit by B 37-42
FLOORS = {"A": 300, "B": 100, "C": 50, "D": 500, "two": 350, "clamped": 150, "B-only": 30}


def channel_sums(terms):
    """(n, 3) integer sums of R, G, B over the terms."""
    return sum(np.stack([(t >> 16) & 0xFF, (t >> 8) & 0xFF, t & 0xFF], axis=1).astype(np.int64) for t in terms)


@pytest.mark.parametrize("algo", ALGOS, ids={oracle.ALGO_ORIGINAL: "ORIGINAL", oracle.ALGO_LONGESTAXIS: "LONGEST_AXIS"}.get)
@pytest.mark.parametrize("store", STORES, ids={oracle.STORE_VCS: "VCS", oracle.STORE_HASHTABLE: "HASH"}.get)
def test_combined_oracle_frames_are_the_reference(store, algo):
    xyz, rgb = lights_cases.golden_voxels()
    longest = algo == oracle.ALGO_LONGESTAXIS
    terms, amb = lights_cases.frame_terms(store, longest)
    ref = oracle.Scene(xyz, rgb, store)
    cam = oracle.reference_camera(W, H)
    frames = [ref.render(algo, cam, lights_ref.fill_block(oracle.lighting(), l), W, H, SCALE)[0] for l in lights_ref.LIGHTS]
    ref.close()
    for name, frame, term in zip("ABCD", frames, terms):
        bad = np.flatnonzero(frame != term)
        assert bad.size == 0, (f"light {name}: {bad.size} of {W * H} pixels differ; first at pixel ({int(bad[0]) % W}, "
                               f"{int(bad[0]) // W}): lights_ref 0x{int(term[bad[0]]):06X} oracle 0x{int(frame[bad[0]]):06X}")
        assert not (frame >> 24).any(), f"light {name}: a term has bits above 23"
    want = lights_ref.combine(frames)
    assert np.array_equal(lights_ref.combine(terms), want)
    # the combination is the definition: per channel min(255, the sum over the lights)
    sums = channel_sums(frames)
    packed = np.minimum(sums, 255).astype(np.uint32)
    assert np.array_equal(want, packed[:, 0] << 16 | packed[:, 1] << 8 | packed[:, 2])
    # shade_lights_rays itself, with and without the ambient term, on every seventh ray
    rays = lights_cases.frame_rays()[::7]
    sc = lights_cases.pyref_scene(store)
    assert np.array_equal(lights_ref.shade_lights_rays(sc, lights_ref.LIGHTS, rays, SCALE, longest), want[::7])
    assert np.array_equal(lights_ref.shade_lights_rays(sc, lights_ref.LIGHTS, rays, SCALE, longest, ambient=lights_ref.AMBIENT),
                          lights_ref.sat_add_rgb(want, amb)[::7])
    assert np.array_equal(lights_ref.shade_lights_rays(sc, (), rays, SCALE, longest), np.zeros(len(rays), np.uint32))
    # the ambient term: at every pixel some unshadowed light could reach (D's frame is a subset of
    # the primary hits), never elsewhere than at a hit, and a quarter of the stored colour
    assert np.count_nonzero(amb) >= FLOORS["D"] and not (amb[frames[3] != 0] == 0).any()
    assert lights_ref.ambient_term(0xFFFFFF, lights_ref.AMBIENT) == 0x3F3F3F
    # the yardsticks
    lit = [f != 0 for f in frames]
    counts = {n: int(np.count_nonzero(l)) for n, l in zip("ABCD", lit)}
    counts["two"] = int(np.count_nonzero(sum(l.astype(int) for l in lit) >= 2))
    counts["clamped"] = int(np.count_nonzero((sums > 255).any(axis=1)))
    counts["B-only"] = int(np.count_nonzero(~lit[0] & lit[1]))
    print(counts)
    for key, floor in FLOORS.items():
        assert counts[key] >= floor, (key, counts)
