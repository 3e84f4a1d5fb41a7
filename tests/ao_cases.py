"""The golden-frame case of vr_occlusion and vr_shade_lights_ao, computed once per (store,
algorithm) and shared by tests/test_ao_ref.py (which keeps it from being vacuous) and
tests/test_gpu_ao.py (which holds the kernels to it): tests/lights_cases.py' 32 x 24 frame of the
golden scene at scale 12, its four lights and ambient term, and the occlusion of its hits."""
from __future__ import annotations

import functools

import numpy as np

from tests import ao_ref, lights_cases, lights_ref, trace_ref

W, H, SCALE = lights_cases.W, lights_cases.H, lights_cases.SCALE


@functools.lru_cache(maxsize=None)
def golden_set():
    return ao_ref.voxel_set(lights_cases.golden_voxels()[0])


@functools.lru_cache(maxsize=None)
def frame_records(store: int, longest: bool):
    """trace_ref's records of the frame's rays (read-only)."""
    recs, _ = trace_ref.trace_rays(lights_cases.pyref_scene(store), lights_cases.frame_rays(), SCALE, longest)
    recs.setflags(write=False)
    return recs


@functools.lru_cache(maxsize=None)
def frame_details(store: int, longest: bool):
    """ao_ref.detail of every record of the frame (None where it is open by definition)."""
    return tuple(ao_ref.detail(golden_set(), r) for r in frame_records(store, longest))


@functools.lru_cache(maxsize=None)
def frame_ao(store: int, longest: bool):
    ao = np.array([d["ao"] if d else ao_ref.OPEN for d in frame_details(store, longest)], dtype=np.uint32)
    ao.setflags(write=False)
    return ao


@functools.lru_cache(maxsize=None)
def frame_words(store: int, longest: bool, strength, apply=ao_ref.AMBIENT, ambient: bool = True):
    """The frame under lights_ref.LIGHTS (and lights_ref.AMBIENT): vr_shade_lights' words for
    strength None, vr_shade_lights_ao's otherwise (read-only)."""
    terms, amb = lights_cases.frame_terms(store, longest)
    if strength is None:
        out = lights_ref.combine(list(terms) + ([amb] if ambient else []))
    else:
        out = ao_ref.apply_ao(terms, amb if ambient else None, frame_ao(store, longest), strength, apply)
    out.setflags(write=False)
    return out
