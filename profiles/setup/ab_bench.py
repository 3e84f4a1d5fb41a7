#!/usr/bin/env python3
"""Interleaved A/B of library builds through bench.py itself: every run a fresh
`bench.py --gpus 1 --config C --steps S` process with VR_LIBRARY naming the build, the builds
taken in turn round by round so that clock drift hits them alike.
  python profiles/setup/ab_bench.py C2[,C4] name=path/libvr.so name=path/other.so [--rounds R] [--steps S] [--full]
Prints `[round] name config ms_per_step` per run (with --full also the lone-launch figures), then per
build and config the median and min-max."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = sys.argv[1:]


def opt(name, default):
    if name in args:
        i = args.index(name)
        v = args[i + 1]
        del args[i:i + 2]
        return v
    return default


rounds, steps = int(opt("--rounds", "1")), opt("--steps", "200")
full = "--full" in args
if full:
    args.remove("--full")
cfgs = args[0].split(",")
builds = [a.split("=", 1) for a in args[1:]]
seen = {}
for rnd in range(rounds):
    for cfg in cfgs:
        for name, lib in builds:
            env = dict(os.environ, VR_LIBRARY=os.path.abspath(lib))
            cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", cfg, "--steps", steps]
            if full:
                cmd += ["--full", "--no-cpu-baseline"]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                print(f"[{rnd}] {name} {cfg} FAILED ({r.returncode}): {r.stderr[-400:]}", flush=True)
                sys.exit(1)       # nothing more on the GPU after a failure
            d = json.loads(r.stdout.strip().splitlines()[-1])
            seen.setdefault((name, cfg), []).append(d["ms_per_step"])
            extra = ""
            if full:
                extra = " " + " ".join(f"{k} {d[k]}" for k in ("kernel_ms", "kernel_ms_grid_order", "kernel_ms_first_render",
                                                               "ms_per_step_moving_view") if k in d)
            print(f"[{rnd}] {name} {cfg} ms_per_step {d['ms_per_step']:.5f}{extra}", flush=True)
for (name, cfg), v in seen.items():
    print(f"{name} {cfg}: median {statistics.median(v):.5f} min {min(v):.5f} max {max(v):.5f} ({len(v)} runs)")
