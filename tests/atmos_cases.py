"""The cases of vr_atmosphere_apply and vr_shade_lights_atmosphere, shared by tests/test_atmos_check.py,
tests/test_atmos_ref.py and tests/test_gpu_atmos.py: an atmosphere whose three sky colours differ and
whose fog runs from 0.25 to 4.0 world units -- the depth-0 hit distances of tests/reflect_cases.py'
golden 32 x 24 frame run from 0.004 to 5.98 with a median of 1.21, so hits lie before the fog, inside
it and past its end -- over that frame's descent (reflect_cases.golden_levels, computed once there)."""
from __future__ import annotations

import functools

import numpy as np

from tests import ao_ref, atmos_ref, reflect_cases

W, H, SCALE = reflect_cases.W, reflect_cases.H, reflect_cases.SCALE
SKY, FOG = atmos_ref.SKY, atmos_ref.FOG
FOG_START, FOG_END = 0.25, 4.0
# (no channel is a multiple of 1/255: every byte is a truncation; up is not of unit length)
ATMOSPHERE = atmos_ref.Atmosphere(zenith=(0.1, 0.3, 0.9), horizon=(0.8, 0.7, 0.6), nadir=(0.35, 0.2, 0.05), up=(0.0, 1.0, 0.0),
                                  fog_color=(0.55, 0.6, 0.7), fog_start=FOG_START, fog_end=FOG_END, flags=SKY | FOG)
# an up that is neither an axis nor of unit length, an inverted ramp
TILTED = atmos_ref.Atmosphere(zenith=(0.0, 0.5, 1.0), horizon=(1.0, 1.0, 1.0), nadir=(0.5, 0.25, 0.0), up=(0.3, 0.8, -0.4),
                              fog_color=(1.0, 0.0, 0.5), fog_start=3.0, fog_end=0.5, flags=SKY | FOG)
# fog_end == fog_start: a step
STEP = atmos_ref.Atmosphere(zenith=(0.2, 0.2, 0.2), horizon=(0.9, 0.1, 0.9), nadir=(0.0, 0.0, 0.0), up=(0.0, 0.0, -2.0),
                            fog_color=(0.0, 1.0, 0.0), fog_start=1.0, fog_end=1.0, flags=SKY | FOG)
FLAGS = (SKY, FOG, SKY | FOG)


def golden_words(store: int, longest: bool, flags: int, k: int, bounces: int, mirror=reflect_cases.EVERY, strength=None,
                 apply=ao_ref.AMBIENT, atm=ATMOSPHERE):
    """vr_shade_lights_atmosphere's words of the golden frame under atm with `flags`."""
    if k == 0:
        bounces = 0
    return atmos_ref.fold(reflect_cases.golden_levels(store, longest, mirror), atm.with_flags(flags), k, bounces, SCALE,
                          strength=strength, apply=apply)


@functools.lru_cache(maxsize=None)
def made_up_words():
    """One colour word per record of reflect_cases.made_up(): every byte value somewhere, bits 24-31
    set in some."""
    n = len(reflect_cases.made_up()[0])
    w = np.random.default_rng(5).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    w[::3] &= np.uint32(0xFFFFFF)
    w.setflags(write=False)
    return w
