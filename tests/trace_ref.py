"""CPU reference of vr_trace and vr_camera_rays, on the pick reference (tests/pick_ref.py, itself
held to the C oracle by tests/test_pick_ref.py): the same PickWalk, started from a given world
ray instead of a pixel's.

  trace_ray   the record of one ray: PickWalk.scene(origin, makeUnitVector(direction), ...),
              assembled exactly as pick_ref.pick_pixel assembles a pixel's record
  camera_ray  vr_camera_rays for one pixel: the image-plane point calculateWorldRay makes and
              the vector it normalises, origin - eye (six quiet NaNs outside the frame)

tests/test_trace_ref.py ties the two to pick_ref.pick_pixel before tests/test_gpu_trace.py uses
them to judge the kernels."""
from __future__ import annotations

import numpy as np

from tests import pick_ref, pyref

MISS, VOXEL, NEVER = pick_ref.MISS, pick_ref.VOXEL, pick_ref.NEVER
HIT_DTYPE = pick_ref.HIT_DTYPE

# vr_ray field for field (tests/test_trace_capi.py: equal to the package's RAY_DTYPE)
RAY_DTYPE = np.dtype([("origin", "<f4", (3,)), ("reserved0", "<u4"), ("direction", "<f4", (3,)), ("reserved1", "<u4")])
QUIET_NAN = 0x7FC00000


def trace_ray(scene, origin, direction, scale, longest, translation=(0.0, 0.0, 0.0)):
    """-> (record of HIT_DTYPE, primary-walk iterations) of the ray from world `origin` along
    `direction` (any length; zero, NaN and infinite values take whatever the walk makes of them)."""
    with np.errstate(all="ignore"):
        w = pick_ref.PickWalk(scene, translation)
        w.scene(pyref.V(*origin), pyref.V(*direction).unit(), scale, longest)
    if w.aborted:
        return pick_ref.record(NEVER), w.iters
    if w.hit is None:
        return pick_ref.record(MISS), w.iters
    color, n, rwp, point, key, cr = w.hit
    r = pick_ref.record(VOXEL)
    r["color"] = color
    local = (key >> 20, (key >> 10) & 1023, key & 1023)
    for i in range(3):
        r["voxel"][i] = pyref.wrap32(pyref.wrap32(cr[i] * pyref.BLOCK) + local[i])
        r["normal"][i] = int(float(n[i]))
        r["region"][i] = cr[i]
        r["point"][i] = point[i]
    return r, w.iters


def trace_rays(scene, rays, scale, longest, translation=(0.0, 0.0, 0.0)):
    """Records (HIT_DTYPE array) and iterations of a RAY_DTYPE array."""
    out = np.zeros(len(rays), dtype=HIT_DTYPE)
    iters = np.zeros(len(rays), dtype=np.int64)
    for i, ray in enumerate(rays):
        out[i], iters[i] = trace_ray(scene, ray["origin"], ray["direction"], scale, longest, translation)
    return out, iters


def camera_ray(cam, W, H, x, y):
    """-> record of RAY_DTYPE: vr_camera_rays for pixel (x, y) of a W x H frame."""
    F = pyref.F
    r = np.zeros((), dtype=RAY_DTYPE)
    if x >= W or y >= H:
        nan = np.array([QUIET_NAN] * 3, dtype=np.uint32).view(np.float32)
        r["origin"], r["direction"] = nan, nan
        return r
    org, llc, hor, ver = cam if isinstance(cam, tuple) else pick_ref.cam_fields(cam)
    u = (F(x) + F(0.5)) / F(W)
    v = (F(pyref.u32(H - y)) + F(0.5)) / F(H)
    ro = (llc + hor.scale(u)) + ver.scale(v)
    d = ro - org
    for i in range(3):
        r["origin"][i] = ro[i]
        r["direction"][i] = d[i]
    return r


def camera_rays(cam, W, H, px, py):
    fields = pick_ref.cam_fields(cam)
    out = np.zeros(len(px), dtype=RAY_DTYPE)
    for i in range(len(px)):
        out[i] = camera_ray(fields, W, H, int(px[i]), int(py[i]))
    return out


def rays_of(origins, directions):
    """A RAY_DTYPE array from (n, 3) origins and directions."""
    o, d = np.asarray(origins, dtype=np.float32), np.asarray(directions, dtype=np.float32)
    out = np.zeros(len(o), dtype=RAY_DTYPE)
    out["origin"], out["direction"] = o, d
    return out
