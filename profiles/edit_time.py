#!/usr/bin/env python3
"""vr_scene_edit against the rebuild it replaces, per config and batch size.

A batch is half inserts at fresh coordinates inside occupied regions and half removals of
stored voxels, device-resident.  Each run applies it with vr_scene_edit (timed), builds the
edited set from scratch with vr_scene_create_ex from device-resident arrays (timed: the
parent's path to the same image), checks that the two digests agree, and undoes the batch
with a second edit (not timed).  Runs are interleaved; times are HIP events on the stream
around each call (both calls return when the scene is ready).  Reports median, min and max
of each, the ratio of the medians, and whether the edit's median is below the rebuild's by
more than the two spreads (max - min) together.

usage: edit_time.py [--runs N] [C2 C5 C4]"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import voxelraymarcher_amd as vr  # noqa: E402

BATCHES = (1, 1000, 100000)


def pack(xyz):
    x = xyz.astype(np.int64) + (1 << 20)
    return (x[:, 0] << 42) | (x[:, 1] << 21) | x[:, 2]


def make_batch(xyz, rgb, n, rng):
    """(exyz, ergb, undo_xyz, undo_rgb, keep mask of the stored voxels)."""
    n_ins = (n + 1) // 2
    n_rem = n - n_ins
    rem = rng.choice(len(xyz), size=n_rem, replace=False)
    stored = np.sort(pack(xyz))
    ins = np.zeros((0, 3), dtype=np.int32)
    while len(ins) < n_ins:          # a stored voxel's region, random local coordinates, not stored
        base = (xyz[rng.integers(0, len(xyz), size=2 * n_ins + 8)] >> 6) << 6
        cand = (base + rng.integers(0, 64, size=base.shape)).astype(np.int32)
        cand = cand[~np.isin(pack(cand), stored)]
        ins = np.unique(np.concatenate([ins, cand]), axis=0)
    ins = ins[rng.permutation(len(ins))[:n_ins]]
    exyz = np.concatenate([ins, xyz[rem]]).astype(np.int32)
    ergb = np.concatenate([rng.integers(0, 1 << 24, size=n_ins, dtype=np.uint32),
                           np.full(n_rem, vr.VOXEL_REMOVE, dtype=np.uint32)])
    undo_rgb = np.concatenate([np.full(n_ins, vr.VOXEL_REMOVE, dtype=np.uint32), rgb[rem]])
    order = rng.permutation(n)
    keep = np.ones(len(xyz), dtype=bool)
    keep[rem] = False
    return exyz[order], ergb[order], exyz[order], undo_rgb[order], keep, ins, ergb[:n_ins]


def dev(a):
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def frame_digest(scene, cfg):
    cam, lit = vr.Camera.reference(cfg.width, cfg.height), vr.setup_constant_values()
    info = vr.VoxelSceneInfo((0.0, 0.0, 0.0), cfg.scale)
    out = vr.run_raymarching_kernel(scene, cfg.algorithm, cam, lit, info, cfg.width, cfg.height)
    torch.cuda.synchronize()
    return hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()


def main():
    args = sys.argv[1:]
    runs = 7
    if "--runs" in args:
        i = args.index("--runs")
        runs = int(args[i + 1])
        del args[i:i + 2]
    torch.cuda.init()
    for name in args or ["C2", "C5", "C4"]:
        cfg = vr.CONFIGS[name]
        xyz, rgb = cfg.voxels()
        rng = np.random.default_rng(0xED17)
        scene = vr.create_scene(dev(xyz), dev(rgb), cfg.store)       # (also the module warm-up)
        digest0 = scene.digest()
        frame0 = frame_digest(scene, cfg) if name == "C2" else None
        for n in BATCHES:
            exyz, ergb, uxyz, urgb, keep, ins, ins_rgb = make_batch(xyz, rgb, n, rng)
            d_exyz, d_ergb, d_uxyz, d_urgb = dev(exyz), dev(ergb), dev(uxyz), dev(urgb)
            d_nxyz = dev(np.concatenate([xyz[keep], ins]).astype(np.int32))
            d_nrgb = dev(np.concatenate([rgb[keep], ins_rgb]))
            scene.edit(d_exyz, d_ergb)                                # warm-up of both paths
            scene.edit(d_uxyz, d_urgb)
            vr.create_scene(d_nxyz, d_nrgb, cfg.store).close()
            t_edit, t_build, same = [], [], True
            for _ in range(runs):
                te, _ = timed(lambda: scene.edit(d_exyz, d_ergb))
                tb, fresh = timed(lambda: vr.create_scene(d_nxyz, d_nrgb, cfg.store))
                same = same and scene.digest() == fresh.digest()
                fresh.close()
                scene.edit(d_uxyz, d_urgb)
                t_edit.append(te)
                t_build.append(tb)
            undone = scene.digest() == digest0
            me, mb = float(np.median(t_edit)), float(np.median(t_build))
            spread = (max(t_edit) - min(t_edit)) + (max(t_build) - min(t_build))
            row = {"config": name, "store": cfg.store.name, "voxels": int(len(rgb)), "edits": n, "runs": runs,
                   "edit_ms": {"median": me, "min": min(t_edit), "max": max(t_edit)},
                   "rebuild_ms": {"median": mb, "min": min(t_build), "max": max(t_build)},
                   "rebuild_over_edit": mb / me, "combined_spread_ms": spread, "edit_wins_by_more_than_spread": mb - me > spread,
                   "digest_equals_rebuild": same, "undo_restores_digest": undone}
            print(json.dumps(row), flush=True)
        if frame0 is not None:
            print(json.dumps({"config": name, "frame_digest_same_after_edit_and_undo": frame_digest(scene, cfg) == frame0,
                              "frame_sha256": frame0}), flush=True)
        scene.close()


if __name__ == "__main__":
    main()
