"""CPU reference of vr_pick: the primary hit behind a pixel, from the Python restatement of
the walks (tests/pyref.py, left as it is).  PickWalk is pyref.Walk with two taps:

  lookup    remembers the last probe that read a stored colour, with the key that matched
            (x << 20 | y << 10 | z, wrapped to 32 bits -- the key both stores compare)
  lighting  is called by a primary hit only, once per walk (the walk runs with shadows off,
            so no shadow walk follows it): its arguments are the hit's stored colour, the
            shading normal, the region's world position and the region-local hit point

The region is the walk's currentRegion list, which grid / grid_la receive and the scene loop
advances in place; (rwp - translation) / 64 gives the same whenever that is exact.  The hit
voxel is region * 64 + the matched key's fields (x = key >> 20, y = (key >> 10) & 1023,
z = key & 1023).  tests/test_pick_ref.py holds this reference to the C oracle before
tests/test_gpu_pick.py uses it to judge the kernel."""
from __future__ import annotations

import numpy as np

from tests import pyref

MISS, VOXEL, NEVER, OUTSIDE = 0, 1, 2, 3

# vr_hit field for field (tests/test_pick_capi.py: equal to the package's HIT_DTYPE)
HIT_DTYPE = np.dtype([("status", "<u4"), ("color", "<u4"), ("voxel", "<i4", (3,)), ("normal", "<i4", (3,)),
                      ("region", "<i4", (3,)), ("point", "<f4", (3,)), ("reserved", "<u4", (2,))])


class PickWalk(pyref.Walk):
    def __init__(self, scene, translation, lit=None):
        lit = pyref.Lighting(shadows=False) if lit is None else lit
        assert not lit.shadows, "a pick walks the primary ray only"
        super().__init__(scene, lit, translation)
        self.last = None        # (matched key, colour) of the last probe that read a stored colour
        self.cr = None          # the walk's currentRegion (the caller's list, advanced in place)
        self.hit = None         # (colour, normal V, rwp V, point V, matched key, region list)

    def lookup(self, reg, x, y, z):
        col = super().lookup(reg, x, y, z)
        if col != pyref.EMPTY:
            self.last = (pyref.u32((pyref.u32(x) << 20) | (pyref.u32(y) << 10) | pyref.u32(z)), col)
        return col

    def grid(self, ray, reg, rwp, cr, shadow):
        self.cr = cr
        return super().grid(ray, reg, rwp, cr, shadow)

    def grid_la(self, orig, reg, rwp, cr, shadow):
        self.cr = cr
        return super().grid_la(orig, reg, rwp, cr, shadow)

    def lighting(self, color, n, rwp, ro):
        if self.hit is None:
            assert self.last is not None and self.last[1] == color
            self.hit = (color, n, rwp, ro, self.last[0], list(self.cr))
        return super().lighting(color, n, rwp, ro)


def cam_fields(cam):
    """(origin, llc, horizontal, vertical) V's of an oracle.OrCamera, a _capi.VrCamera or a vr.Camera."""
    raw = getattr(cam, "raw", cam)
    return (pyref.V(*raw.origin), pyref.V(*raw.lower_left), pyref.V(*raw.horizontal), pyref.V(*raw.vertical))


def record(status=MISS):
    r = np.zeros((), dtype=HIT_DTYPE)
    r["status"] = status
    return r


def pick_pixel(scene, cam, W, H, x, y, scale, longest, translation=(0.0, 0.0, 0.0), lit=None):
    """-> (record of HIT_DTYPE, primary-walk iterations, the PickWalk): calculateWorldRay
    (Renderer.cuh:1013-1022) and the primary walk of pixel (x, y), as pyref.render_pixel makes them."""
    F = pyref.F
    if x >= W or y >= H:
        return record(OUTSIDE), 0, None
    org, llc, hor, ver = cam if isinstance(cam, tuple) else cam_fields(cam)
    u = (F(x) + F(0.5)) / F(W)
    v = (F(pyref.u32(H - y)) + F(0.5)) / F(H)
    ro = (llc + hor.scale(u)) + ver.scale(v)
    with np.errstate(divide="ignore", invalid="ignore"):
        rd = (ro - org).unit()
    w = PickWalk(scene, translation, lit)
    w.scene(ro, rd, scale, longest)
    if w.aborted:
        return record(NEVER), w.iters, w
    if w.hit is None:
        return record(MISS), w.iters, w
    color, n, rwp, point, key, cr = w.hit
    r = record(VOXEL)
    r["color"] = color
    local = (key >> 20, (key >> 10) & 1023, key & 1023)
    for i in range(3):
        r["voxel"][i] = pyref.wrap32(pyref.wrap32(cr[i] * pyref.BLOCK) + local[i])
        r["normal"][i] = int(float(n[i]))
        r["region"][i] = cr[i]
        r["point"][i] = point[i]
    return r, w.iters, w


def pick_pixels(scene, cam, W, H, px, py, scale, longest, translation=(0.0, 0.0, 0.0)):
    """Records (HIT_DTYPE array) and primary-walk iterations of a list of pixels."""
    fields = cam_fields(cam)
    out = np.zeros(len(px), dtype=HIT_DTYPE)
    iters = np.zeros(len(px), dtype=np.int64)
    for i in range(len(px)):
        out[i], iters[i], _ = pick_pixel(scene, fields, W, H, int(px[i]), int(py[i]), scale, longest, translation)
    return out, iters


def shade(scene, rec, lit, translation=(0.0, 0.0, 0.0)):
    """The pixel a render without shadows writes for a record: applyLighting (pyref.Walk.lighting)
    from the record's fields alone for VOXEL, 0 otherwise."""
    if int(rec["status"]) != VOXEL:
        return 0
    assert not lit.shadows
    F = pyref.F
    w = pyref.Walk(scene, lit, translation)
    rwp = w.tr + pyref.V(*[pyref.wrap32(int(c) * pyref.BLOCK) for c in rec["region"]])
    n = pyref.V(*[F(int(c)) for c in rec["normal"]])
    return w.lighting(int(rec["color"]), n, rwp, pyref.V(*[F(c) for c in rec["point"]]))


def same_records(a, b):
    """Field-by-field equality of two HIT_DTYPE arrays, `point` by its bits with any NaN equal
    to any NaN; -> indices that differ."""
    a, b = np.asarray(a), np.asarray(b)
    bad = np.zeros(a.shape, dtype=bool)
    for f in ("status", "color", "voxel", "normal", "region", "reserved"):
        d = a[f] != b[f]
        bad |= d.reshape(len(a), -1).any(axis=1) if d.ndim > 1 else d
    pa, pb = a["point"], b["point"]
    eq = (pa.view(np.uint32) == pb.view(np.uint32)) | (np.isnan(pa) & np.isnan(pb))
    bad |= ~eq.all(axis=1)
    return np.flatnonzero(bad)
