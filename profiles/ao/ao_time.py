#!/usr/bin/env python3
"""vr_occlusion against the cheapest thing a caller could do before it -- vr_scene_lookup of the
same 8 n neighbour coordinates, before any host arithmetic -- and vr_shade_lights_ao against
vr_shade_lights.  A 1920 x 1080 frame's hits per config, everything device-resident;
times are HIP events on the stream around each call (every call here returns when its work is
done), 7 interleaved runs after a warm-up, medians with their ranges.

occlusion  the frame's records (vr_trace of its camera rays, 8 x 8-tile order) through vr_occlusion,
           and the 8 n coordinates of their neighbours (the plane cell itself for a record that is
           no hit) through vr_scene_lookup, alternating; a record whose lookups find no neighbour
           must be open in vr_occlusion's values.
lights     vr_shade_lights and vr_shade_lights_ao (strength 255, both modes, with ao_out) for the
           same rays at L = 1 and L = 4 lights with an ambient term, alternating.

usage: ao_time.py [--runs N] [occlusion|lights ...]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import voxelraymarcher_amd as vr  # noqa: E402

WIDTH, HEIGHT = 1920, 1080
CELLS = ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))
TANGENTS = ((1, 2), (2, 0), (0, 1))


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


def frame(name):
    cfg = vr.CONFIGS[name]
    xyz, rgb = cfg.voxels()
    scene = vr.create_scene(dev(xyz), dev(rgb), cfg.store)
    tw, th = WIDTH // 8, HEIGHT // 8
    y = torch.arange(HEIGHT, dtype=torch.int32, device="cuda").view(th, 1, 8, 1).expand(th, tw, 8, 8).reshape(-1).contiguous()
    x = torch.arange(WIDTH, dtype=torch.int32, device="cuda").view(1, tw, 1, 8).expand(th, tw, 8, 8).reshape(-1).contiguous()
    rays = vr.camera_rays(vr.Camera.reference(WIDTH, HEIGHT), WIDTH, HEIGHT, x, y)
    return cfg, scene, rays, vr.VoxelSceneInfo((0.0, 0.0, 0.0), cfg.scale)


def neighbour_coordinates(recs):
    """(8 n, 3) int32: per record the eight cells around voxel + normal in the face's plane (eight
    times the plane cell for a record without a unit axis normal)."""
    vox, nrm = recs["voxel"].astype(np.int64), recs["normal"].astype(np.int64)
    axis = np.argmax(np.abs(nrm), axis=1)
    out = np.repeat((vox + nrm)[:, None, :], 8, axis=1)
    live = (recs["status"] == 1) & (np.abs(nrm).sum(axis=1) == 1)
    for a in range(3):
        rows = live & (axis == a)
        u, w = TANGENTS[a]
        out[rows, :, u] += np.array([c[0] for c in CELLS])
        out[rows, :, w] += np.array([c[1] for c in CELLS])
    return np.ascontiguousarray(out.reshape(-1, 3).astype(np.int32)), live


def occlusion_against_lookups(name, runs):
    cfg, scene, rays, info = frame(name)
    drecs = vr.trace(scene, cfg.algorithm, info, rays)
    recs = drecs.cpu().numpy().view(vr.HIT_DTYPE).reshape(-1)
    q, live = neighbour_coordinates(recs)
    d_q = dev(q)
    ao = vr.occlusion(scene, drecs).cpu().numpy().view(np.uint32)           # warm-up of both paths
    occ = (scene.lookup(d_q).cpu().numpy() != -1).reshape(-1, 8)
    # a record that is no hit, or whose lookups find no neighbour, is open
    assert (ao[~live] == 255).all() and (ao[live & ~occ.any(axis=1)] == 255).all()
    t_ao, t_lk = [], []
    for _ in range(runs):
        t_ao.append(timed(lambda: vr.occlusion(scene, drecs))[0])
        t_lk.append(timed(lambda: scene.lookup(d_q))[0])
    ma, ml = float(np.median(t_ao)), float(np.median(t_lk))
    print(json.dumps({"what": "occlusion", "config": name, "store": cfg.store.name, "records": int(len(recs)),
                      "voxel_hits": int(live.sum()), "occluded": int((ao < 255).sum()), "runs": runs,
                      "occlusion_ms": stats(t_ao), "lookup_8n_ms": stats(t_lk), "lookup_over_occlusion": ml / ma,
                      "ranges_overlap": not (max(t_ao) < min(t_lk) or max(t_lk) < min(t_ao))}), flush=True)
    scene.close()


def lights_with_and_without(name, runs):
    cfg, scene, rays, info = frame(name)
    base = vr.setup_constant_values()
    more = [vr.setup_constant_values(light_direction=d, light_color=c)
            for d, c in (((-2.0, 1.0, 3.0), (0.5, 0.75, 1.0)), ((1.0, 2.0, 3.0), (1.0, 0.5, 0.25)), ((0.3, 1.0, -0.2), (0.4, 0.4, 0.4)))]
    amb = (0.25, 0.25, 0.25)
    for lights in ([base], [base] + more):
        calls = {"shade_lights": lambda: vr.shade_lights(scene, cfg.algorithm, info, lights, rays, ambient=amb),
                 "ao_ambient": lambda: vr.shade_lights(scene, cfg.algorithm, info, lights, rays, ambient=amb, ao=255, return_ao=True),
                 "ao_all": lambda: vr.shade_lights(scene, cfg.algorithm, info, lights, rays, ambient=amb, ao=255,
                                                   ao_apply=vr.AoApply.ALL, return_ao=True)}
        for fn in calls.values():
            fn()                                                            # warm-up
        t = {k: [] for k in calls}
        for _ in range(runs):
            for k, fn in calls.items():
                t[k].append(timed(fn)[0])
        print(json.dumps({"what": "lights", "config": name, "store": cfg.store.name, "rays": int(rays.shape[0]),
                          "lights": len(lights), "runs": runs, "ms": {k: stats(v) for k, v in t.items()},
                          "ao_ambient_over_plain": float(np.median(t["ao_ambient"]) / np.median(t["shade_lights"])),
                          "ao_all_over_plain": float(np.median(t["ao_all"]) / np.median(t["shade_lights"]))}), flush=True)
    scene.close()


def main():
    args = sys.argv[1:]
    runs = 7
    if "--runs" in args:
        i = args.index("--runs")
        runs = int(args[i + 1])
        del args[i:i + 2]
    parts = args or ["occlusion", "lights"]
    torch.cuda.init()
    for name in ("C2", "C4"):
        if "occlusion" in parts:
            occlusion_against_lookups(name, runs)
        if "lights" in parts:
            lights_with_and_without(name, runs)


if __name__ == "__main__":
    main()
