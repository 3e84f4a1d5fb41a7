"""The launch decisions (csrc/vr_launch_plan.h: the launch policy, the crawl-pass skip's state
machine, the learned orders' match and remake rules) are pure functions; the stand-alone
program csrc/tools/launch_plan_check.cpp checks them against literal tables on a CPU."""
from __future__ import annotations

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launch_plan_check():
    exe = os.path.join(ROOT, "voxelraymarcher_amd", "bin", "launch_plan_check")
    assert os.path.exists(exe), "build with make -C voxelraymarcher_amd/csrc"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
