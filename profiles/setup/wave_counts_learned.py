#!/usr/bin/env python3
"""profiles/wave_counts.py for the steady state: the counting build's wave-level counters of ONE
launch of the view after `--warmup` launches of it, so that the launch runs under the learned lane
and work orders as bench.py's timed launches do (wave_counts.py counts the view's second launch,
which still runs the 8 x 8 tiles in grid order).
  VR_LIBRARY=voxelraymarcher_amd/libvr_cover.so python profiles/setup/wave_counts_learned.py [C2] [--warmup 40]"""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import voxelraymarcher_amd as vr  # noqa: E402
from voxelraymarcher_amd import _capi  # noqa: E402
from tests.cover_run import GUARDS, N_COUNTERS  # noqa: E402

args = sys.argv[1:]
warm = 40
if "--warmup" in args:
    i = args.index("--warmup")
    warm = int(args[i + 1])
    del args[i:i + 2]
name = args[0] if args else "C2"
cfg = vr.CONFIGS[name]
xyz, rgb = cfg.voxels()
scene = vr.create_scene(xyz, rgb, cfg.store)
W, H = cfg.width, cfg.height
cam, lit, info = vr.Camera.reference(W, H), vr.setup_constant_values(), vr.VoxelSceneInfo((0, 0, 0), cfg.scale)
out = torch.empty(W * H, dtype=torch.int32, device="cuda")
lib = _capi.lib()
lib.vr_diag_fetch.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]
lib.vr_diag_fetch.restype = ctypes.c_int
buf = (ctypes.c_uint64 * N_COUNTERS)()
before = vr.debug_order_uses(scene.info()["device"])
for _ in range(warm):
    vr.run_raymarching_kernel(scene, cfg.algorithm, cam, lit, info, W, H, out)
    torch.cuda.synchronize()
assert lib.vr_diag_fetch(buf, 1) == 0
vr.run_raymarching_kernel(scene, cfg.algorithm, cam, lit, info, W, H, out)
assert lib.vr_diag_fetch(buf, 1) == 0
after = vr.debug_order_uses(scene.info()["device"])
waves = ((W + 7) // 8) * ((H + 7) // 8)
print(f"{name} {W}x{H}: {waves} waves, one launch after {warm}; lane order uses {after['lane_order_uses'] - before['lane_order_uses']}, "
      f"work order uses {after['work_order_uses'] - before['work_order_uses']}")
for k in range(N_COUNTERS):
    if buf[k]:
        print(f"  [{k:2d}] {GUARDS.get(k, ('?',))[0]:60s} {buf[k]:12d}  ({buf[k] / waves:8.2f} per wave)")
