"""vr_shade of a full frame's camera rays against vr_trace of the same rays and against a first
render of the same view (profiles/shade/README.md).

    python profiles/shade_time.py C2 [--rounds 15]

Per config, one JSON line with median / min / max in ms.  Every sample is one HIP event pair
around one call, with vr_forget_orders before it (so the render is a first render: 8x8 tiles, no
learned order); shade and trace end in their own stream synchronise, so their samples hold that
host round trip, and the render's sample is waited for in the same way.  All variants alternate
within each round, after 3 warm-up rounds.  Rays, colours, records and the frame are on the
device.  The rays come in two orders: row-major (64 pixels of one row per wave) and 8x8-tile
order (tiles row-major, pixels row-major in a tile: the render's wave).

  shade_given / shade_coherent      vr_shade, hits NULL, under GIVEN and under COHERENT (key
                                    kernel and sort included)
  shade_hits_given                  vr_shade with the records
  trace_given                       vr_trace of the same rays
  render_first                      vr_render of the same view after vr_forget_orders

The script also checks that every shade has the words of the render and that the records are
the trace's."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import voxelraymarcher_amd as vr  # noqa: E402

WARM = 3
GIVEN, COHERENT = vr.TraceOrder.GIVEN, vr.TraceOrder.COHERENT


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def timed(fn):
    vr.forget_orders(0)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def measure(name: str, rounds: int):
    cfg = vr.CONFIGS[name]
    xyz, rgb = cfg.voxels()
    W, H = cfg.width, cfg.height
    assert W % 8 == 0 and H % 8 == 0
    scene = vr.create_scene(xyz, rgb, cfg.store)
    del xyz, rgb
    cam = vr.Camera.reference(W, H)
    info = vr.VoxelSceneInfo((0.0, 0.0, 0.0), cfg.scale)
    lit = vr.setup_constant_values()
    i = np.arange(W * H, dtype=np.int64)
    t, k = i // 64, i % 64
    tx, ty = (t % (W // 8)) * 8 + k % 8, (t // (W // 8)) * 8 + k // 8
    order = {"row": (i % W, i // W), "tile": (tx, ty)}
    pix = {key: tuple(torch.from_numpy(a.astype(np.int32)).cuda() for a in v) for key, v in order.items()}
    rays = {key: vr.camera_rays(cam, W, H, *pix[key]) for key in pix}
    at = {key: (pix[key][1].to(torch.int64) * W + pix[key][0].to(torch.int64)) for key in pix}
    frame = torch.empty(W * H, dtype=torch.int32, device="cuda")

    def render():
        vr.run_raymarching_kernel(scene, cfg.algorithm, cam, lit, info, W, H, frame)
        torch.cuda.synchronize()
        return frame

    calls = {"render_first": render}
    for key in ("row", "tile"):
        r = rays[key]
        calls[f"shade_given_{key}"] = lambda r=r: vr.shade(scene, cfg.algorithm, info, lit, r, order=GIVEN)
        calls[f"shade_coherent_{key}"] = lambda r=r: vr.shade(scene, cfg.algorithm, info, lit, r, order=COHERENT)
        calls[f"shade_hits_given_{key}"] = lambda r=r: vr.shade(scene, cfg.algorithm, info, lit, r, order=GIVEN, hits=True)
        calls[f"trace_given_{key}"] = lambda r=r: vr.trace(scene, cfg.algorithm, info, r, order=GIVEN)
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
    same = True
    for key in ("row", "tile"):
        want = frame[at[key]]
        same &= bool(torch.equal(last[f"shade_given_{key}"], want) and torch.equal(last[f"shade_coherent_{key}"], want))
        same &= bool(torch.equal(last[f"shade_hits_given_{key}"][0], want))
        same &= bool(torch.equal(last[f"shade_hits_given_{key}"][1], last[f"trace_given_{key}"]))
    res["shade_is_render"] = same
    res["lit_pixels"] = int((frame != 0).sum())
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
