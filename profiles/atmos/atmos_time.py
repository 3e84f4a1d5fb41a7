#!/usr/bin/env python3
"""vr_shade_lights_atmosphere against the call without an atmosphere and against the same result composed
from public parts on the device.  A 1920 x 1080 frame's rays in 8 x 8-tile order per config,
one light and an ambient term, reflectivity 96, everything device-resident; times are HIP events on
the stream around each call or composition (every call here returns when its work is done),
interleaved runs after a warm-up, medians with their ranges.

reflect      shade_lights(reflect=96, bounces=B): no atmosphere -- the null path, which launches what
             the parent commit launches
atmosphere   the same call with atmosphere= (SKY | FOG)
composition  per depth shade_lights(hits=True) over EVERY ray, atmosphere_apply over its words, rays
             and records, bounce_rays, and at the end the blend in torch integer ops masked by what
             reflects: only integer ops are torch's, so its words must equal the call's exactly
apply        atmosphere_apply alone over the frame's rays, depth-0 records and words
copy         a device-to-device copy of the colour buffer (4 bytes per ray): the yardstick for what
             an elementwise pass over the colours must cost at least

--reflect-only times `reflect` alone and uses nothing this commit adds, so that the same script runs
against the parent commit's package (--package ROOT: import voxelraymarcher_amd from ROOT).

usage: atmos_time.py [--runs N] [--reflect-only] [--package ROOT] [C2 C4 ...]"""
import json
import os
import sys

import numpy as np
import torch

WIDTH, HEIGHT = 1920, 1080
K = 96
vr = None


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


def mix_torch(a, b, k):
    out = torch.zeros_like(a)
    for sh in (16, 8, 0):
        out |= ((((a >> sh) & 0xFF) * (255 - k) + ((b >> sh) & 0xFF) * k + 127) // 255) << sh
    return out


def composed(scene, algo, info, lights, amb, rays, atm, k, bounces):
    cols, refls = [], []
    alive = torch.ones(rays.shape[0], dtype=torch.bool, device=rays.device)
    cur = rays
    for j in range(bounces + 1):
        c, h = vr.shade_lights(scene, algo, info, lights, cur, ambient=amb, hits=True)
        a = vr.atmosphere_apply(cur, h, c, info, atm)
        cols.append(torch.where(alive, a, torch.zeros_like(a)))
        if j < bounces:
            alive = alive & (h[:, 0] == 1)
            refls.append(alive)
            cur = vr.bounce_rays(cur, h, info)
    out = cols[bounces]
    for j in range(bounces - 1, -1, -1):
        out = torch.where(refls[j], mix_torch(cols[j], out, k), cols[j])
    return out


def config(name, runs, reflect_only):
    cfg = vr.CONFIGS[name]
    xyz, rgb = cfg.voxels()
    tw, th = WIDTH // 8, HEIGHT // 8
    y = torch.arange(HEIGHT, dtype=torch.int32, device="cuda").view(th, 1, 8, 1).expand(th, tw, 8, 8).reshape(-1).contiguous()
    x = torch.arange(WIDTH, dtype=torch.int32, device="cuda").view(1, tw, 1, 8).expand(th, tw, 8, 8).reshape(-1).contiguous()
    rays = vr.camera_rays(vr.Camera.reference(WIDTH, HEIGHT), WIDTH, HEIGHT, x, y)
    info = vr.VoxelSceneInfo((0.0, 0.0, 0.0), cfg.scale)
    lights, amb = [vr.setup_constant_values()], (0.25, 0.25, 0.25)
    scene = vr.create_scene(dev(xyz), dev(rgb), cfg.store)
    algo = cfg.algorithm
    for bounces in (1, 2):
        calls = {"reflect": lambda: vr.shade_lights(scene, algo, info, lights, rays, ambient=amb, reflect=K, bounces=bounces)}
        extra = {}
        if not reflect_only:
            # the fog's ramp over the distances of the frame's first hits: their 10th to 90th percentile
            c0, h0 = vr.shade_lights(scene, algo, info, lights, rays, ambient=amb, hits=True)
            hit = h0[:, 0] == 1
            p = (h0[:, 8:11].float() * 64.0 + h0[:, 11:14].view(torch.float32)) / float(cfg.scale)      # (translation 0)
            dist = (p - rays[:, 0:3]).norm(dim=1)[hit]
            lo, hi = (float(q) for q in torch.quantile(dist[:: max(1, dist.numel() // 100000)], torch.tensor([0.1, 0.9], device="cuda")))
            atm = vr.Atmosphere(fog_start=lo, fog_end=hi, flags=vr.Atmosphere.SKY | vr.Atmosphere.FOG)
            dst = torch.empty_like(c0)
            calls["atmosphere"] = lambda: vr.shade_lights(scene, algo, info, lights, rays, ambient=amb, reflect=K, bounces=bounces,
                                                          atmosphere=atm)
            calls["composition"] = lambda: composed(scene, algo, info, lights, amb, rays, atm, K, bounces)
            calls["apply"] = lambda: vr.atmosphere_apply(rays, h0, c0, info, atm)
            calls["copy"] = lambda: dst.copy_(c0)
            got, want, plain = calls["atmosphere"](), calls["composition"](), calls["reflect"]()
            extra = {"misses_at_depth_0": int((h0[:, 0] == 0).sum()), "hits_at_depth_0": int(hit.sum()), "fog_start": lo, "fog_end": hi,
                     "words_changed": int((got != plain).sum()), "composition_differs": int((got != want).sum())}
        for fn in calls.values():        # warm-up
            fn()
        t = {k: [] for k in calls}
        for _ in range(runs):
            for k, fn in calls.items():
                t[k].append(timed(fn)[0])
        m = {k: float(np.median(v)) for k, v in t.items()}
        if not reflect_only:
            extra.update(atmosphere_minus_reflect_ms=m["atmosphere"] - m["reflect"],
                         atmosphere_over_composition=m["atmosphere"] / m["composition"],
                         added_over_copies=(m["atmosphere"] - m["reflect"]) / ((bounces + 1) * m["copy"]))
        print(json.dumps({"what": "atmosphere", "config": name, "store": cfg.store.name, "rays": int(rays.shape[0]), "bounces": bounces,
                          "runs": runs, "ms": {k: stats(v) for k, v in t.items()}, **extra}), flush=True)
    scene.close()


def main():
    global vr
    args = sys.argv[1:]
    runs, root = 7, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if "--runs" in args:
        i = args.index("--runs")
        runs = int(args[i + 1])
        del args[i:i + 2]
    if "--package" in args:
        i = args.index("--package")
        root = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    reflect_only = "--reflect-only" in args
    args = [a for a in args if a != "--reflect-only"]
    sys.path.insert(0, root)
    import voxelraymarcher_amd
    vr = voxelraymarcher_amd
    torch.cuda.init()
    for name in (args or ["C2", "C4"]):
        config(name, runs, reflect_only)


if __name__ == "__main__":
    main()
