"""vr_shade_lights of a full frame's camera rays under L lights against the way a caller had to do
it before: L calls of vr_shade into L buffers and a saturating byte-wise add in torch (DESIGN 4i,
profiles/lights/README.md).

    python profiles/lights/lights_time.py C2 C4 [--rounds 15]

Per config, one JSON line with median / min / max in ms for L in {1, 2, 4, 8}.  Every sample is one
HIP event pair around one variant: for `lights`, one vr_shade_lights call (it ends in its own
stream synchronise); for `baseline`, the L vr_shade calls (each ends in its own synchronise) and
the torch add, then a synchronise.  The variants alternate within each round, after 3 warm-up
rounds.  Rays (1920 x 1080, 8x8-tile order: tiles row-major, pixels row-major in a tile) and
colours are on the device.  The lights have distinct directions: light 0 is the default light,
the others directional with shadows on.

The script also checks, at every L, that the two ways give the same words."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import voxelraymarcher_amd as vr  # noqa: E402

WARM = 3
COUNTS = (1, 2, 4, 8)
# un-normalised directions of lights 1..7 (light 0: the default (1, 1, 1)), all with a positive y
DIRECTIONS = [(-2.0, 1.0, 3.0), (1.0, 2.0, 3.0), (3.0, 1.0, -2.0), (-1.0, 3.0, -1.0), (-3.0, 2.0, 0.5), (0.5, 1.0, -3.0),
              (2.0, 3.0, 1.0)]
COLORS = [(0.5, 0.75, 1.0), (1.0, 1.0, 1.0), (1.0, 0.5, 0.25), (0.25, 0.5, 0.25), (0.5, 0.5, 0.5), (0.75, 0.25, 1.0),
          (0.3, 0.3, 0.3)]


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def sat_add(terms):
    """min(255, sum) per channel of int32 word tensors, bits 24-31 dropped: the caller's own add."""
    out = None
    for sh in (16, 8, 0):
        s = sum((t >> sh) & 0xFF for t in terms).clamp_(max=255) << sh
        out = s if out is None else out | s
    return out


def measure(name: str, rounds: int):
    cfg = vr.CONFIGS[name]
    xyz, rgb = cfg.voxels()
    W, H = 1920, 1080
    scene = vr.create_scene(xyz, rgb, cfg.store)
    del xyz, rgb
    cam = vr.Camera.reference(W, H)
    info = vr.VoxelSceneInfo((0.0, 0.0, 0.0), cfg.scale)
    lights = [vr.setup_constant_values()]
    lights += [vr.setup_constant_values(light_direction=d, light_color=c) for d, c in zip(DIRECTIONS, COLORS)]
    i = np.arange(W * H, dtype=np.int64)
    t, k = i // 64, i % 64
    px = torch.from_numpy(((t % (W // 8)) * 8 + k % 8).astype(np.int32)).cuda()
    py = torch.from_numpy(((t // (W // 8)) * 8 + k // 8).astype(np.int32)).cuda()
    rays = vr.camera_rays(cam, W, H, px, py)

    calls = {}
    for n in COUNTS:
        ls = lights[:n]
        calls[f"lights_{n}"] = lambda ls=ls: vr.shade_lights(scene, cfg.algorithm, info, ls, rays)

        def baseline(ls=ls):
            out = sat_add([vr.shade(scene, cfg.algorithm, info, l, rays) for l in ls])
            torch.cuda.synchronize()
            return out
        calls[f"baseline_{n}"] = baseline
    samples = {v: [] for v in calls}
    last = {}
    for r in range(WARM + rounds):
        for v, fn in calls.items():
            ms, last[v] = timed(fn)
            if r >= WARM:
                samples[v].append(ms)
    res = {"config": name, "rays": W * H, "rounds": rounds}
    for v in calls:
        res[v] = stats(samples[v])
    res["same_words"] = all(bool(torch.equal(last[f"lights_{n}"], last[f"baseline_{n}"])) for n in COUNTS)
    res["lit_pixels"] = {n: int((last[f"lights_{n}"] != 0).sum()) for n in COUNTS}
    print(json.dumps(res), flush=True)
    scene.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="+")
    ap.add_argument("--rounds", type=int, default=15)
    args = ap.parse_args()
    assert args.rounds >= 7
    for name in args.configs:
        measure(name, args.rounds)
