#!/usr/bin/env python3
"""vr_scene_paint against vr_scene_edit, the render after each, and vr_scene_lookup's rate
(DESIGN 4h).  Times are HIP events on the stream around each call (every call here returns
when its work is done), 7 interleaved runs after a warm-up, inputs device-resident.

paint    per config and batch size: the identical recolour batch (distinct stored voxels, new
         colours) through vr_scene_paint and through vr_scene_edit, alternating; each pair is
         checked to leave the same digest.
after    C2 at its bench size: the view is rendered until it is under its learned orders, then
         one visible voxel is recoloured -- through paint, through edit, or not at all -- and
         the next render is timed.  (After an edit the view is learned again before the next
         run.)
lookup   per config, 2 073 600 queries: a dense box (coherent: neighbouring lanes ask for
         neighbouring voxels) and a shuffle of stored voxels and as many absent ones.

usage: access_time.py [--runs N] [paint|after|lookup ...]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import voxelraymarcher_amd as vr  # noqa: E402

BATCHES = (1, 1000, 100000)
QUERIES = 1920 * 1080


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


def paint_against_edit(name, runs):
    cfg = vr.CONFIGS[name]
    xyz, rgb = cfg.voxels()
    rng = np.random.default_rng(0xACCE55)
    scene = vr.create_scene(dev(xyz), dev(rgb), cfg.store)
    for n in BATCHES:
        n = min(n, len(xyz))
        at = rng.choice(len(xyz), size=n, replace=False)
        d_xyz = dev(np.ascontiguousarray(xyz[at]))
        colours = [dev(rng.integers(0, 1 << 24, size=n, dtype=np.uint32)) for _ in range(2)]
        assert scene.paint(d_xyz, colours[0]) == 0                     # warm-up of both paths
        scene.edit(d_xyz, colours[1])
        t_paint, t_edit, same = [], [], True
        for k in range(runs):
            tp, absent = timed(lambda: scene.paint(d_xyz, colours[k & 1]))
            painted = scene.digest()
            te, _ = timed(lambda: scene.edit(d_xyz, colours[k & 1]))
            same = same and absent == 0 and scene.digest() == painted
            t_paint.append(tp)
            t_edit.append(te)
        mp, me = float(np.median(t_paint)), float(np.median(t_edit))
        spread = (max(t_paint) - min(t_paint)) + (max(t_edit) - min(t_edit))
        print(json.dumps({"what": "paint", "config": name, "store": cfg.store.name, "voxels": int(len(rgb)), "edits": n,
                          "runs": runs, "paint_ms": stats(t_paint), "edit_ms": stats(t_edit), "edit_over_paint": me / mp,
                          "combined_spread_ms": spread, "paint_wins_by_more_than_spread": me - mp > spread,
                          "digest_equals_edit": same}), flush=True)
    scene.close()


def render_after(name, runs):
    cfg = vr.CONFIGS[name]
    xyz, rgb = cfg.voxels()
    scene = vr.create_scene(dev(xyz), dev(rgb), cfg.store)
    device = scene.info()["device"]
    cam, lit = vr.Camera.reference(cfg.width, cfg.height), vr.setup_constant_values()
    info = vr.VoxelSceneInfo((0.0, 0.0, 0.0), cfg.scale)
    out = torch.empty(cfg.width * cfg.height, dtype=torch.int32, device="cuda")

    def render():
        vr.run_raymarching_kernel(scene, cfg.algorithm, cam, lit, info, cfg.width, cfg.height, out=out)

    def learn():
        for _ in range(vr.debug_order_uses(device)["slots"] + 2):
            render()
            torch.cuda.synchronize()

    ys, xs = np.mgrid[cfg.height // 18:cfg.height:cfg.height // 9, cfg.width // 32:cfg.width:cfg.width // 16]
    hits = scene.pick(cfg.algorithm, cam, info, cfg.width, cfg.height, xs.reshape(-1), ys.reshape(-1))
    hits = hits[hits["status"] == int(vr.HitStatus.VOXEL)]
    assert len(hits), "no pixel of the 16 x 9 grid shows a voxel"
    d_xyz = dev(hits["voxel"][len(hits) // 2].astype(np.int32).reshape(1, 3))
    colours = [dev(np.array([c], dtype=np.uint32)) for c in (0x00FF00, 0xFF00FF)]
    learn()
    t = {"unchanged": [], "after_paint": [], "after_edit": []}
    bound = {"after_paint": 0, "after_edit": 0}
    for k in range(runs + 1):                                           # (run 0 is the warm-up)
        rows = {"unchanged": timed(render)[0]}
        for what, change in (("after_paint", scene.paint), ("after_edit", scene.edit)):
            change(d_xyz, colours[k & 1])
            before = vr.debug_order_uses(device)["lane_order_uses"]
            rows[what] = timed(render)[0]
            bound[what] += (vr.debug_order_uses(device)["lane_order_uses"] - before) if k else 0
            if what == "after_edit":
                learn()
        if k:
            for what, ms in rows.items():
                t[what].append(ms)
    print(json.dumps({"what": "after", "config": name, "size": [cfg.width, cfg.height], "runs": runs,
                      "render_ms": {what: stats(v) for what, v in t.items()},
                      "renders_with_lane_order_bound": bound}), flush=True)
    scene.close()


def lookup_rate(name, runs):
    cfg = vr.CONFIGS[name]
    xyz, rgb = cfg.voxels()
    rng = np.random.default_rng(0x100C)
    scene = vr.create_scene(dev(xyz), dev(rgb), cfg.store)
    side = int(round(QUERIES ** (1 / 3))) + 1
    lo = np.median(xyz, axis=0).astype(np.int64) - side // 2
    box = (np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[:QUERIES] + lo).astype(np.int32)
    half = QUERIES // 2
    stored = xyz[rng.integers(0, len(xyz), size=half)]
    absent = stored[rng.permutation(half)] ^ np.array([1, 0, 0], dtype=np.int32)      # (mostly absent neighbours)
    mixed = np.concatenate([stored, absent])[rng.permutation(2 * half)].astype(np.int32)
    for kind, q in (("dense_box", box), ("shuffled_stored_and_absent", mixed)):
        d_q = dev(np.ascontiguousarray(q))
        found = int((scene.lookup(d_q) != -1).sum())                    # warm-up
        t = [timed(lambda: scene.lookup(d_q))[0] for _ in range(runs)]
        print(json.dumps({"what": "lookup", "config": name, "store": cfg.store.name, "queries": int(len(q)), "kind": kind,
                          "found": found, "runs": runs, "ms": stats(t),
                          "queries_per_us": len(q) / (float(np.median(t)) * 1e3)}), flush=True)
    scene.close()


def main():
    args = sys.argv[1:]
    runs = 7
    if "--runs" in args:
        i = args.index("--runs")
        runs = int(args[i + 1])
        del args[i:i + 2]
    parts = args or ["paint", "after", "lookup"]
    torch.cuda.init()
    if "paint" in parts:
        for name in ("C2", "C5", "C4"):
            paint_against_edit(name, runs)
    if "after" in parts:
        render_after("C2", runs)
    if "lookup" in parts:
        for name in ("C2", "C4"):
            lookup_rate(name, runs)


if __name__ == "__main__":
    main()
