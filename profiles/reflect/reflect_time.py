#!/usr/bin/env python3
"""vr_shade_lights_reflect against the same result composed from the public calls that existed
before it, with torch ops on the device.  A 1920 x 1080 frame's rays in 8 x 8-tile order
per config, everything device-resident; times are HIP events on the stream around each call or
composition (every call here returns when its work is done), interleaved runs after a warm-up,
medians with their ranges.

call         shade_lights(reflect=96, bounces=B, mirror=M) for B = 1, 2
composition  per depth shade_lights(hits=True) over EVERY ray, the bounce rays from its records in
             torch (the hit point back in world units, the direction's sign flipped on the normal's
             axis), and at the end the blend in torch integer ops, masked by what reflects -- what a
             caller did before, without the host round trip (which would only add to it)
plain        shade_lights alone: what either adds is on top of this

Mirror tests: every voxel; the material bit (colour & 1) == 1; a key colour painted on every
hundredth voxel (about 1 % of them) under mask 0xFFFFFF.  The composition's words are compared with
the call's before anything is timed, and the count of differing words is reported (torch's float
arithmetic is not bound to the call's operation order).

usage: reflect_time.py [--runs N] [C2 C4 ...]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import voxelraymarcher_amd as vr  # noqa: E402

WIDTH, HEIGHT = 1920, 1080
K = 96
KEY = 0x00FF7F


def dev(a):
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stats(t):
    return {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))}


def bounce_torch(rays, hits, info):
    """The bounce rays of (n, 8) float32 rays at (n, 16) int32 records, in torch."""
    tr = torch.tensor(info.translation, dtype=torch.float32, device=rays.device)
    region, point = hits[:, 8:11].float(), hits[:, 11:14].view(torch.float32)
    n = hits[:, 5:8].abs().float()
    out = torch.zeros_like(rays)
    out[:, 0:3] = tr + (region * 64.0 + point) / float(info.scale)
    out[:, 4:7] = rays[:, 4:7] * (1.0 - 2.0 * n)
    return out


def mix_torch(a, b, k):
    out = torch.zeros_like(a)
    for sh in (16, 8, 0):
        out |= ((((a >> sh) & 0xFF) * (255 - k) + ((b >> sh) & 0xFF) * k + 127) // 255) << sh
    return out


def composed(scene, algo, info, lights, amb, rays, k, bounces, mirror):
    cols, refls = [], []
    alive = torch.ones(rays.shape[0], dtype=torch.bool, device=rays.device)
    cur = rays
    for j in range(bounces + 1):
        if j < bounces:
            c, h = vr.shade_lights(scene, algo, info, lights, cur, ambient=amb, hits=True)
            alive = alive & (h[:, 0] == 1) & ((h[:, 1] & mirror[0]) == mirror[1])
            refls.append(alive)
            # (a ray that is not alive keeps a finite ray: its word is masked out below)
            cur = torch.where(alive[:, None], bounce_torch(cur, h, info), cur)
        else:
            c = vr.shade_lights(scene, algo, info, lights, cur, ambient=amb)
        cols.append(c)
    out = cols[bounces]
    for j in range(bounces - 1, -1, -1):
        out = torch.where(refls[j], mix_torch(cols[j], out, k), cols[j])
    return out


def config(name, runs):
    cfg = vr.CONFIGS[name]
    xyz, rgb = cfg.voxels()
    tw, th = WIDTH // 8, HEIGHT // 8
    y = torch.arange(HEIGHT, dtype=torch.int32, device="cuda").view(th, 1, 8, 1).expand(th, tw, 8, 8).reshape(-1).contiguous()
    x = torch.arange(WIDTH, dtype=torch.int32, device="cuda").view(1, tw, 1, 8).expand(th, tw, 8, 8).reshape(-1).contiguous()
    rays = vr.camera_rays(vr.Camera.reference(WIDTH, HEIGHT), WIDTH, HEIGHT, x, y)
    info = vr.VoxelSceneInfo((0.0, 0.0, 0.0), cfg.scale)
    lights, amb = [vr.setup_constant_values()], (0.25, 0.25, 0.25)
    scene = vr.create_scene(dev(xyz), dev(rgb), cfg.store)
    for label, mirror in (("every", (0, 0)), ("bit", (1, 1)), ("key", (0xFFFFFF, KEY))):
        if label == "key":
            stored = set(rgb.tolist())
            key = next(c for c in range(KEY, 1 << 24) if c not in stored)       # a colour the scene does not store
            mirror = (0xFFFFFF, key)
            which = np.arange(0, len(xyz), 100)
            scene.paint(np.ascontiguousarray(xyz[which]), np.full(len(which), key, dtype=np.uint32))
        for bounces in (1, 2):
            calls = {"plain": lambda: vr.shade_lights(scene, cfg.algorithm, info, lights, rays, ambient=amb),
                     "call": lambda: vr.shade_lights(scene, cfg.algorithm, info, lights, rays, ambient=amb, reflect=K,
                                                     bounces=bounces, mirror=mirror),
                     "composition": lambda: composed(scene, cfg.algorithm, info, lights, amb, rays, K, bounces, mirror)}
            got, want, plain = calls["call"](), calls["composition"](), calls["plain"]()        # warm-up
            _, h = vr.shade_lights(scene, cfg.algorithm, info, lights, rays, ambient=amb, hits=True)
            reflecting = int(((h[:, 0] == 1) & ((h[:, 1] & mirror[0]) == mirror[1])).sum())
            t = {k: [] for k in calls}
            for _ in range(runs):
                for k, fn in calls.items():
                    t[k].append(timed(fn)[0])
            m = {k: float(np.median(v)) for k, v in t.items()}
            print(json.dumps({"what": "reflect", "config": name, "store": cfg.store.name, "rays": int(rays.shape[0]),
                              "mirror": label, "bounces": bounces, "reflecting_at_depth_0": reflecting,
                              "words_changed": int((got != plain).sum()), "composition_differs": int((got != want).sum()),
                              "runs": runs, "ms": {k: stats(v) for k, v in t.items()},
                              "call_over_composition": m["call"] / m["composition"],
                              "call_minus_plain_ms": m["call"] - m["plain"],
                              "ranges_overlap": not (max(t["call"]) < min(t["composition"]) or max(t["composition"]) < min(t["call"]))}),
                  flush=True)
    scene.close()


def main():
    args = sys.argv[1:]
    runs = 7
    if "--runs" in args:
        i = args.index("--runs")
        runs = int(args[i + 1])
        del args[i:i + 2]
    torch.cuda.init()
    for name in (args or ["C2", "C4"]):
        config(name, runs)


if __name__ == "__main__":
    main()
