"""The closed-form fast-forward of cluster-skip crawls (csrc/vr_crawl.h: crawl_steps,
crawl_run, crawl_voxel) against a plain single-step loop, o <- o + RN(EPSILON d) per
component in float32, over >= 20 000 seeded adversarial starts: the three axes pinned on
the cluster planes 0..56, coordinates next to powers of two, cluster faces, integers and
zero, steps below an ulp, ties from odd and even mantissas, crawls through the region's
absent clusters.  bin/crawl_check (csrc/tools/crawl_check.hip) generates the cases, runs
the header -- its host compile with --cpu, its device compile (one lane per case)
otherwise -- and the loop, and prints the counts asserted here.

Measured (MI355X, device compile; the host compile gives the same counts): 20 005 cases,
2.3e8 loop iterations; no wrong prefix, no short count, no capped run; 20 % / 7 % of the
runs (without / with cluster bits) are empty, 22 % / 26 % end by themselves; 4498 of 4542
and 4862 of 4913 long runs take <= 1 % trips; crawl_steps applied in 12 766 cases;
crawl_voxel ambiguous for 0 random, 104 near-integer and 0 pinned inputs, never wrong.
The tool runs 0.8 s (0.4 s of it the host loop)."""
from __future__ import annotations

import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "voxelraymarcher_amd", "bin", "crawl_check")


def run_tool(*args):
    assert os.path.exists(EXE), "build with make -C voxelraymarcher_amd/csrc"
    r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode in (0, 1), r.stderr          # anything else: it crashed
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(res))
    return r.returncode, res, r.stderr


def check(rc, res, stderr, mode):
    assert res["mode"] == mode
    assert res["cases"] >= 20_000
    for name in ("plain", "cluster_bits"):           # crawl_run without / with the cluster bits
        m = res[name]
        assert m["runs"] == res["cases"]
        # the generator (the loop's counts alone): few empty crawls, enough that end by themselves
        assert m["zero_share"] <= 0.30, (name, m)
        assert m["self_end_share"] >= 0.20, (name, m)
        # 1. exact prefix  2. complete, but for the trip cap
        assert m["over_room"] == 0, (name, m, stderr)
        assert m["bad_prefix"] == 0, (name, m, stderr)
        assert m["incomplete"] == 0, (name, m, stderr)
        assert m["capped"] <= 0.01 * m["runs"], (name, m)
        # 3. long crawls take <= 1 % of their iterations in trips
        assert m["long_runs"] >= 1000, (name, m)
        assert m["long_fast"] >= 0.95 * m["long_runs"], (name, m)
    # 4. crawl_steps alone
    assert res["steps"]["applied"] >= 1000, res["steps"]
    assert res["steps"]["bad"] == 0, (res["steps"], stderr)
    # crawl_voxel: the voxel of the position before the step, or ambiguity
    v = res["voxel"]
    assert (v["random"], v["integer"], v["pinned"]) == (200_000, 20_000, 28)
    assert v["random_wrong"] == v["integer_wrong"] == v["pinned_wrong"] == 0, (v, stderr)
    assert v["random_ambiguous"] < 50, v
    assert v["pinned_ambiguous"] == 0, v
    assert res["ok"] is True and rc == 0


def test_crawl_fast_forward_host_compile():
    check(*run_tool("--cpu"), "cpu")


@pytest.mark.gpu
def test_crawl_fast_forward_device_compile():
    check(*run_tool(), "device")
