"""vr_trace against vr_pick, and its execution orders against each other (DESIGN 4f,
profiles/trace/README.md).

    python profiles/trace_time.py C2 C4 [--rounds 15]

Per config, JSON lines with median / min / max in ms.  Every sample is one HIP event pair around
one call, with vr_forget_orders before it; a call ends in its own stream synchronise, so the
sample holds that host round trip as well.  All variants of a table alternate within each round,
after 3 warm-up rounds.  Rays, pixels and records are on the device.

(a) "vs_pick": the camera rays of all W x H pixels traced in the GIVEN order against vr_pick of
    the same pixels, in row-major order and in 8x8-tile order (tiles row-major, pixels
    row-major in a tile).
(b) "orders": GIVEN against COHERENT (key kernel and sort included) on the first n rays of
      tile      the tile-order camera rays (already coherent)
      shuffled  the same rays under a seeded shuffle
      bounce    one ray per VOXEL record of the frame's pick (tile order): origin the hit point
                in world space, translation + (region * 64 + point) / scale, direction the
                record's normal plus a seeded random unit vector
      bounce_u  the same with the origin translation + region * 64 + point, the lighting's
                unscaled world point: at a scale other than 1 these start far outside the scene
    for n = 2^12, 2^14, ... and the whole set.
The script also checks that trace(camera_rays) has the bytes of the pick and that both orders
give the same records on every set."""
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
    i = np.arange(W * H, dtype=np.int64)
    t, k = i // 64, i % 64
    tx, ty = (t % (W // 8)) * 8 + k % 8, (t // (W // 8)) * 8 + k // 8
    order = {"row": (i % W, i // W), "tile": (tx, ty)}
    pix = {key: tuple(torch.from_numpy(a.astype(np.int32)).cuda() for a in v) for key, v in order.items()}
    rays = {key: vr.camera_rays(cam, W, H, *pix[key]) for key in pix}

    # ---- (a) trace GIVEN against pick, order by order
    variants = {f"{kind}_{key}": None for key in ("row", "tile") for kind in ("pick", "trace")}
    samples = {v: [] for v in variants}
    last = {}
    for r in range(WARM + rounds):
        for key in ("row", "tile"):
            ms_p, last[f"pick_{key}"] = timed(lambda: vr.pick(scene, cfg.algorithm, cam, info, W, H, *pix[key]))
            ms_t, last[f"trace_{key}"] = timed(lambda: vr.trace(scene, cfg.algorithm, info, rays[key], order=GIVEN))
            if r >= WARM:
                samples[f"pick_{key}"].append(ms_p)
                samples[f"trace_{key}"].append(ms_t)
    res = {"config": name, "table": "vs_pick", "rays": W * H, "rounds": rounds}
    for v in variants:
        res[v] = stats(samples[v])
    res["trace_is_pick"] = bool(all(torch.equal(last[f"pick_{key}"], last[f"trace_{key}"]) for key in ("row", "tile")))
    print(json.dumps(res), flush=True)

    # ---- (b) the ray sets
    recs = last["pick_tile"].cpu().numpy().view(vr.HIT_DTYPE).reshape(-1)
    hit = recs[recs["status"] == vr.HitStatus.VOXEL]
    rng = np.random.default_rng(1)
    u = rng.normal(size=(len(hit), 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    scene_point = hit["region"].astype(np.float32) * np.float32(64.0) + hit["point"]
    bounce = np.zeros((2, len(hit), 8), dtype=np.float32)
    bounce[0, :, 0:3] = scene_point / np.float32(cfg.scale)
    bounce[1, :, 0:3] = scene_point
    bounce[:, :, 4:7] = (hit["normal"].astype(np.float32) + u.astype(np.float32))[None]
    perm = torch.from_numpy(np.random.default_rng(2).permutation(W * H)).cuda()
    sets = {"tile": rays["tile"], "shuffled": rays["tile"][perm].contiguous(),
            "bounce": torch.from_numpy(bounce[0]).cuda(), "bounce_u": torch.from_numpy(bounce[1]).cuda()}
    for key, full in sets.items():
        sizes = [n for n in (1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20) if n < full.shape[0]] + [full.shape[0]]
        for n in sizes:
            sub = full[:n].contiguous()
            samples = {GIVEN: [], COHERENT: []}
            out = {}
            for r in range(WARM + rounds):
                for o in (GIVEN, COHERENT):
                    ms, out[o] = timed(lambda: vr.trace(scene, cfg.algorithm, info, sub, order=o))
                    if r >= WARM:
                        samples[o].append(ms)
            st = out[GIVEN][:, 0]
            res = {"config": name, "table": "orders", "set": key, "rays": n, "rounds": rounds,
                   "given": stats(samples[GIVEN]), "coherent": stats(samples[COHERENT]),
                   "orders_agree": bool(torch.equal(out[GIVEN], out[COHERENT])),
                   "voxel_records": int((st == int(vr.HitStatus.VOXEL)).sum())}
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
