"""CPU reference of vr_shade_lights: several of the reference's lights and an ambient term for
any rays, from tests/shade_ref.py and tests/pyref.py (both left as they are).

  sat_add_rgb        the byte-wise sum of two words with a clamp at 255 per channel, bits 24-31
                     of either word dropped
  ambient_term       the directional formula of pyref.Walk.lighting with diff = 1 and the light's
                     colour replaced by `ambient`, in float32 through pyref's to_vec / to_int:
                     to_int(to_vec(col) * ambient), as a 32-bit word
  shade_lights_rays  shade_ref.shade_rays once per light (light_color filled into
                     pyref.Lighting.LC), the ambient term at every primary VOXEL hit
                     (trace_ref.trace_rays), and the combination

tests/test_lights_ref.py ties it to the C oracle's frames before tests/test_gpu_lights.py uses it
to judge the kernels.  A light is a plain tuple (use_shadows, use_point_light, light_pos,
light_dir un-normalised or None for (1, 1, 1), light_color): shade_ref.LIGHTINGS' form plus a
colour, so that the lighting blocks of a test (pyref's, the oracle's, libvr's) are filled from
the same floats."""
from __future__ import annotations

import numpy as np

from tests import pyref, shade_ref, trace_ref

F = np.float32

# the four lights of the golden-frame tests
LIGHT_A = (True, False, (10.0, 10.0, -10.0), None, (1.0, 1.0, 1.0))                  # the default light
LIGHT_B = (True, False, (10.0, 10.0, -10.0), (-2.0, 1.0, 3.0), (0.5, 0.75, 1.0))
LIGHT_C = (True, True, (40.0, 90.0, 30.0), None, (1.0, 1.0, 1.0))                    # a point light
LIGHT_D = (False, False, (10.0, 10.0, -10.0), (1.0, 2.0, 3.0), (1.0, 1.0, 1.0))      # unshadowed
LIGHTS = (LIGHT_A, LIGHT_B, LIGHT_C, LIGHT_D)
AMBIENT = (0.25, 0.25, 0.25)


def sat_add_rgb(a, b):
    """min(255, R(a) + R(b)) << 16 | min(255, G(a) + G(b)) << 8 | min(255, B(a) + B(b)) of uint32
    words or arrays."""
    a, b = np.asarray(a, dtype=np.uint32), np.asarray(b, dtype=np.uint32)
    out = np.zeros(np.broadcast(a, b).shape, dtype=np.uint32)
    for sh in (16, 8, 0):
        s = ((a >> np.uint32(sh)) & np.uint32(0xFF)) + ((b >> np.uint32(sh)) & np.uint32(0xFF))
        out |= np.minimum(s, np.uint32(255)).astype(np.uint32) << np.uint32(sh)
    return out if out.shape else np.uint32(out)


def ambient_term(col: int, ambient) -> int:
    """The ambient term of a voxel whose stored colour is col: each channel
    f2u((c / 255 * ambient[ch]) * 255) in float32, packed R << 16 | G << 8 | B in 32 bits."""
    with np.errstate(all="ignore"):
        return int(pyref.Walk.to_int(pyref.Walk.to_vec(int(col)).mul(pyref.V(*ambient)))) & 0xFFFFFFFF


def pyref_light(light):
    shadows, point, pos, direction, color = light
    lit = shade_ref.pyref_lighting(shadows, point, pos, direction)
    lit.LC = pyref.V(*color)
    return lit


def fill_block(block, light):
    """Write a light into a C lighting block that holds its defaults (oracle.OrLighting or the
    package's VrLighting), as shade_ref.fill_block does, and its colour."""
    shade_ref.fill_block(block, *light[:4])
    for i in range(3):
        block.light_color[i] = float(light[4][i])
    return block


def light_terms(scene, lights, rays, scale, longest, translation=(0.0, 0.0, 0.0)):
    """One uint32 array per light: the word vr_shade writes for each ray under it."""
    return [shade_ref.shade_rays(scene, pyref_light(l), rays, scale, longest, translation)[0] for l in lights]


def ambient_terms(scene, ambient, rays, scale, longest, translation=(0.0, 0.0, 0.0)):
    """The ambient term of every ray: ambient_term of the stored colour at a primary VOXEL hit, 0
    for a miss and for a primary walk that never ends."""
    recs, _ = trace_ref.trace_rays(scene, rays, scale, longest, translation)
    out = np.zeros(len(rays), dtype=np.uint32)
    memo = {}
    for i in np.flatnonzero(recs["status"] == trace_ref.VOXEL):
        c = int(recs["color"][i])
        if c not in memo:
            memo[c] = ambient_term(c, ambient)
        out[i] = memo[c]
    return out


def combine(terms):
    """The words of vr_shade_lights from its terms (uint32 arrays of one length, at least one)."""
    out = np.zeros_like(np.asarray(terms[0], dtype=np.uint32))
    for t in terms:
        out = sat_add_rgb(out, t)
    return out


def shade_lights_rays(scene, lights, rays, scale, longest, translation=(0.0, 0.0, 0.0), ambient=None):
    """The uint32 words vr_shade_lights writes for a RAY_DTYPE array."""
    terms = light_terms(scene, lights, rays, scale, longest, translation)
    if ambient is not None:
        terms.append(ambient_terms(scene, ambient, rays, scale, longest, translation))
    return combine(terms) if terms else np.zeros(len(rays), dtype=np.uint32)
