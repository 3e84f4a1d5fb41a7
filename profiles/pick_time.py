"""vr_pick over every pixel of a config's frame against a first render of the same view
without shadows (profiles/pick/README.md).

    python profiles/pick_time.py C2 C4 [--rounds 15]

Per config, one JSON line: median / min / max in ms of
  row     vr_pick of all W x H pixels in row-major order, queries and records on the device
  tile    the same pixels in 8x8-tile order (tiles row-major, pixels row-major in a tile)
  render  a first render of the view with shadows off: vr_forget_orders before every launch
          (bench.py --full's kernel_ms_first_render method), one HIP event pair around 20
          launches, divided by 20
vr_forget_orders precedes every pick too.  A pick sample is one HIP event pair around one call;
the call ends in its own stream synchronise, so the sample holds that host round trip as well.
The three variants alternate within each round, after 3 warm-up rounds.  The script also checks
that both orders give the same records and that every lit pixel has a VOXEL record."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import voxelraymarcher_amd as vr  # noqa: E402

WARM, RENDERS = 3, 20


def measure(name: str, rounds: int) -> dict:
    cfg = vr.CONFIGS[name]
    xyz, rgb = cfg.voxels()
    W, H = cfg.width, cfg.height
    assert W % 8 == 0 and H % 8 == 0
    scene = vr.create_scene(xyz, rgb, cfg.store)
    del xyz, rgb
    cam = vr.Camera.reference(W, H)
    info = vr.VoxelSceneInfo((0.0, 0.0, 0.0), cfg.scale)
    lit = vr.setup_constant_values(use_shadows=False)
    i = np.arange(W * H, dtype=np.int64)
    t, k = i // 64, i % 64
    tx, ty = (t % (W // 8)) * 8 + k % 8, (t // (W // 8)) * 8 + k // 8
    order = {"row": (i % W, i // W), "tile": (tx, ty)}
    dev = {key: tuple(torch.from_numpy(a.astype(np.int32)).cuda() for a in v) for key, v in order.items()}
    frame = torch.empty(W * H, dtype=torch.int32, device="cuda")

    def events():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def time_pick(key):
        vr.forget_orders(0)
        a, b = events()
        a.record()
        hits = vr.pick(scene, cfg.algorithm, cam, info, W, H, *dev[key])
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), hits

    def time_render():
        a, b = events()
        a.record()
        for _ in range(RENDERS):
            vr.forget_orders(0)
            vr.run_raymarching_kernel(scene, cfg.algorithm, cam, lit, info, W, H, out=frame)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / RENDERS

    samples = {"row": [], "tile": [], "render": []}
    for r in range(WARM + rounds):
        ms_row, h_row = time_pick("row")
        ms_tile, h_tile = time_pick("tile")
        ms_render = time_render()
        if r >= WARM:
            samples["row"].append(ms_row)
            samples["tile"].append(ms_tile)
            samples["render"].append(ms_render)
    h_row, h_tile, lit_frame = h_row.cpu().numpy(), h_tile.cpu().numpy(), frame.cpu().numpy()
    scene.close()
    res = {"config": name, "pixels": W * H, "rounds": rounds}
    for key, v in samples.items():
        res[key] = {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    res["orders_agree"] = bool(np.array_equal(h_row[ty * W + tx], h_tile))
    res["lit_pixels_have_a_voxel"] = bool((h_row[lit_frame != 0, 0] == vr.HitStatus.VOXEL).all())
    res["voxel_records"] = int((h_row[:, 0] == vr.HitStatus.VOXEL).sum())
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="+")
    ap.add_argument("--rounds", type=int, default=15)
    args = ap.parse_args()
    assert args.rounds >= 7
    for name in args.configs:
        print(json.dumps(measure(name, args.rounds)), flush=True)
