"""CPU reference of vr_shade: the colour a render writes for a pixel whose ray is a given world
ray -- pyref.Walk (tests/pyref.py, left as it is), started from the ray instead of from a pixel:

  shade_ray   pyref.Walk(scene, lit, translation).scene(origin, makeUnitVector(direction), ...):
              applyLighting at the primary hit times !shadow, 0 for a miss and 0 for a primary or
              shadow walk that never ends (as pyref.render_pixel writes it)

tests/test_shade_ref.py ties it to the C oracle's frames -- shade_ray of trace_ref.camera_rays
is oracle.Scene.render, under every lighting of LIGHTINGS -- before tests/test_gpu_shade.py uses
it to judge the kernel.  The lightings are kept as plain values, so that the three lighting
blocks of a test (pyref's, the oracle's, libvr's) are filled from the same floats."""
from __future__ import annotations

import numpy as np

from tests import pyref


def shade_walk(scene, lit, origin, direction, scale, longest, translation=(0.0, 0.0, 0.0)):
    """-> (colour, the walk never ends) of the ray from world `origin` along `direction`."""
    with np.errstate(all="ignore"):
        w = pyref.Walk(scene, lit, translation)
        col = w.scene(pyref.V(*origin), pyref.V(*direction).unit(), scale, longest)
    return (0 if w.aborted else int(col)), bool(w.aborted)


def shade_ray(scene, lit, origin, direction, scale, longest, translation=(0.0, 0.0, 0.0)):
    """The word vr_shade writes for the ray: 0 when the walk aborted."""
    return shade_walk(scene, lit, origin, direction, scale, longest, translation)[0]


def shade_rays(scene, lit, rays, scale, longest, translation=(0.0, 0.0, 0.0)):
    """(uint32 colours, bool never-ends) of a RAY_DTYPE array."""
    col = np.zeros(len(rays), dtype=np.uint32)
    never = np.zeros(len(rays), dtype=bool)
    for i, ray in enumerate(rays):
        col[i], never[i] = shade_walk(scene, lit, ray["origin"], ray["direction"], scale, longest, translation)
    return col, never


def unit3(d):
    """makeUnitVector(d) in float32 (Vector3.cuh:162-165), as three Python floats."""
    with np.errstate(all="ignore"):
        return tuple(float(c) for c in pyref.V(*d).unit())


# name -> (use_shadows, use_point_light, light_pos, light_dir un-normalised or None for (1, 1, 1))
LIGHTINGS = {
    "directional": (True, False, (10.0, 10.0, -10.0), None),
    "directional-unshadowed": (False, False, (10.0, 10.0, -10.0), None),
    "directional-123": (True, False, (10.0, 10.0, -10.0), (1.0, 2.0, 3.0)),
    "point": (True, True, (40.0, 90.0, 30.0), None),
}


def pyref_lighting(shadows, point, pos, direction=None):
    lit = pyref.Lighting(shadows=shadows, point=point, pos=pos)
    if direction is not None:
        lit.L = pyref.V(*unit3(direction))
    return lit


def fill_block(block, shadows, point, pos, direction=None):
    """Write a lighting into a C lighting block (oracle.OrLighting or the package's VrLighting,
    already holding its defaults): light_dir is the float32 makeUnitVector of `direction`."""
    block.use_shadows, block.use_point_light = int(shadows), int(point)
    for i in range(3):
        block.light_pos[i] = float(pos[i])
    if direction is not None:
        for i, c in enumerate(unit3(direction)):
            block.light_dir[i] = c
    return block


def unshadowed(spec):
    return (False,) + tuple(spec[1:])
