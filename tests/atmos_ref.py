"""CPU reference of vr_atmosphere_apply and vr_shade_lights_atmosphere (include/vr.h): the
sky and the distance fog in numpy, written from the header's text and built only on
tests/reflect_ref.py (left as it is).

  Atmosphere  the fields of vr_atmosphere
  byte, pack  a colour byte of a float channel, a colour's word
  q256        a fraction as 0..256
  lerp256     two words blended by q in 0..256, in integers
  sky         the sky's word in the direction of every ray
  fog         every word under the fog of its record's distance
  atmos       atmos(w, ray, record) for arrays of one length
  fold        the words of vr_shade_lights_atmosphere from reflect_ref.descend's levels

Every float operation is one float32 operation, in the header's order.  tests/test_atmos_check.py
holds atmos to the C++ arithmetic (bin/atmos_check), tests/test_atmos_ref.py keeps the cases from
being vacuous, tests/test_gpu_atmos.py judges the kernels by it."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests import ao_ref, reflect_ref

F = np.float32
MISS, VOXEL = 0, reflect_ref.VOXEL
SKY, FOG = 1, 2


@dataclass(frozen=True)
class Atmosphere:
    zenith: tuple
    horizon: tuple
    nadir: tuple
    up: tuple = (0.0, 1.0, 0.0)
    fog_color: tuple = (0.5, 0.5, 0.5)
    fog_start: float = 0.0
    fog_end: float = 1.0
    flags: int = SKY | FOG

    def with_flags(self, flags: int) -> "Atmosphere":
        return Atmosphere(self.zenith, self.horizon, self.nadir, self.up, self.fog_color, self.fog_start, self.fog_end, int(flags))

    def floats(self) -> np.ndarray:
        """The 17 floats in vr_atmosphere's order."""
        return np.array(list(self.zenith) + list(self.horizon) + list(self.nadir) + list(self.up) + list(self.fog_color)
                        + [self.fog_start, self.fog_end], dtype=F)


def byte(x) -> int:
    """min(255, f2u(x * 255.0f)): NaN and values <= 0 give 0, everything else truncates."""
    with np.errstate(all="ignore"):
        f = F(x) * F(255.0)
    if np.isnan(f) or f <= 0:
        return 0
    return 255 if f >= 255 else int(f)


def pack(c) -> int:
    return byte(c[0]) << 16 | byte(c[1]) << 8 | byte(c[2])


def q256(f) -> np.ndarray:
    """g = f * 256.0f; 0 if !(g > 0) (NaN too), 256 if g >= 256, else (int)g."""
    with np.errstate(all="ignore"):
        g = (np.asarray(f, dtype=F) * F(256.0)).astype(F)
        inside = (g > 0) & (g < 256)
        return np.where(g >= 256, 256, np.where(inside, np.where(inside, g, 0).astype(np.int64), 0)).astype(np.int64)


def lerp256(a, b, q) -> np.ndarray:
    """Each of the bytes R, G, B is (A * (256 - q) + B * q + 128) >> 8; bits 24-31 are dropped."""
    a, b = np.asarray(a, dtype=np.uint32).astype(np.int64), np.asarray(b, dtype=np.uint32).astype(np.int64)
    q = np.asarray(q, dtype=np.int64)
    out = np.zeros(np.broadcast(a, b, q).shape, dtype=np.int64)
    for sh in (16, 8, 0):
        out |= ((((a >> sh) & 0xFF) * (256 - q) + ((b >> sh) & 0xFF) * q + 128) >> 8) << sh
    return out.astype(np.uint32)


def _len3(v) -> np.ndarray:
    """sqrtf((x*x + y*y) + z*z), every operation rounded to float32."""
    x, y, z = (v[:, c].astype(F) for c in range(3))
    return np.sqrt((((x * x).astype(F) + (y * y).astype(F)).astype(F) + (z * z).astype(F)).astype(F)).astype(F)


def sky_h(atm: Atmosphere, rays) -> np.ndarray:
    """h of every ray: ((d.x*up.x + d.y*up.y) + d.z*up.z) / len."""
    d = np.ascontiguousarray(rays["direction"]).astype(F)
    up = np.asarray(atm.up, dtype=F)
    with np.errstate(all="ignore"):
        dot = (((d[:, 0] * up[0]).astype(F) + (d[:, 1] * up[1]).astype(F)).astype(F) + (d[:, 2] * up[2]).astype(F)).astype(F)
        return (dot / _len3(d)).astype(F)


def sky(atm: Atmosphere, rays) -> np.ndarray:
    h = sky_h(atm, rays)
    with np.errstate(all="ignore"):
        toward = np.where(h < 0, np.uint32(pack(atm.nadir)), np.uint32(pack(atm.zenith)))
        return lerp256(np.uint32(pack(atm.horizon)), toward, q256(np.abs(h)))


def fog_distance(rays, recs, scale, translation=(0.0, 0.0, 0.0)) -> np.ndarray:
    """D of every (ray, record) pair: the record's point back in world space (vr_bounce_rays' origin,
    for every record) minus the ray's origin, and its length."""
    with np.errstate(all="ignore"):
        m = (recs["region"].astype(F) * F(64.0)).astype(F)
        s = (m + recs["point"]).astype(F)
        q = (s / F(np.uint32(scale))).astype(F)
        p = (np.asarray(translation, dtype=F) + q).astype(F)
        e = (p - np.ascontiguousarray(rays["origin"]).astype(F)).astype(F)
        return _len3(e)


def fog_q(atm: Atmosphere, rays, recs, scale, translation=(0.0, 0.0, 0.0)) -> np.ndarray:
    with np.errstate(all="ignore"):
        span = F(F(atm.fog_end) - F(atm.fog_start))
        D = fog_distance(rays, recs, scale, translation)
        return q256(((D - F(atm.fog_start)).astype(F) / span).astype(F))


def fog(atm: Atmosphere, w, rays, recs, scale, translation=(0.0, 0.0, 0.0)) -> np.ndarray:
    return lerp256(w, np.uint32(pack(atm.fog_color)), fog_q(atm, rays, recs, scale, translation))


def atmos(atm: Atmosphere, w, rays, recs, scale, translation=(0.0, 0.0, 0.0)) -> np.ndarray:
    """atmos(w[i], rays[i], recs[i]): the sky for a MISS under SKY, the fog for a VOXEL record under
    FOG, w bit for bit for everything else."""
    w = np.asarray(w, dtype=np.uint32)
    assert len(w) == len(rays) == len(recs)
    out = w.copy()
    if len(w) == 0:
        return out
    status = recs["status"]
    if atm.flags & SKY:
        m = status == MISS
        out[m] = sky(atm, rays)[m]
    if atm.flags & FOG:
        m = status == VOXEL
        out[m] = fog(atm, w, rays, recs, scale, translation)[m]
    return out


def fold(levels, atm: Atmosphere | None, k: int, bounces: int, scale, translation=(0.0, 0.0, 0.0), strength=None,
         apply=ao_ref.AMBIENT) -> np.ndarray:
    """colors of vr_shade_lights_atmosphere from reflect_ref.descend's levels: reflect_ref.fold with
    A^j = atmos(W^j, ray^j, H^j) in the place of W^j.  atm None or flags 0: reflect_ref.fold."""
    if atm is None or atm.flags == 0:
        return reflect_ref.fold(levels, k, bounces, strength, apply)
    levels = levels[: int(bounces) + 1]
    n = len(levels[0].idx)
    deep = None
    for j in range(len(levels) - 1, -1, -1):
        lv = levels[j]
        c = np.zeros(n, dtype=np.uint32)
        c[lv.idx] = atmos(atm, reflect_ref.level_words(lv, strength, apply), lv.rays, lv.recs, scale, translation)
        if deep is not None:
            r = lv.idx[lv.refl]
            c[r] = reflect_ref.mix(c[r], deep[r], k)
        deep = c
    return deep
