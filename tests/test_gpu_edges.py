"""GPU parity at the guard edges of the walk kernels: the directed cases of tests/edge_cases.py
(whose CPU preconditions tests/test_edge_cases.py asserts), every store x algorithm, held to the
oracle as the fuzz holds its cases (check_frame: counted and uncounted launches, pixels and
algorithmic bytes bit-exact, relaunches under learned orders); vr.pick over every pixel of the
E1, E3 and E5 cases; and the proof that the guards these cases aim at really ran, from the
counting build of the library (libvr_cover.so) in one child process."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from tests import edge_cases as ec
from tests import pick_ref, pyref
from tests.cover_run import GUARDS, UNREACHABLE, gpu_camera, gpu_lighting
from tests.helpers import oracle_camera_from, oracle_lighting_from
from tests.test_gpu_parity import ALGOS, STORES, check_frame

pytestmark = pytest.mark.gpu

vr = pytest.importorskip("voxelraymarcher_amd")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COVER_LIB = os.path.join(ROOT, "voxelraymarcher_amd", "libvr_cover.so")


@pytest.mark.parametrize("name", list(ec.CASES))
def test_edge_views(name):
    c = ec.CASES[name]
    cam, lit = gpu_camera(c), gpu_lighting(c)
    assert np.array_equal(np.array(lit.light_dir[:], dtype=np.float32), ec.light(c))
    for store in [s for s in STORES if int(s) in c.stores]:
        ref = oracle.Scene(c.xyz, c.rgb, int(store))
        gpu = vr.create_scene(c.xyz, c.rgb, store)
        for algo in ALGOS:
            want = ref.render(int(algo), oracle_camera_from(cam), oracle_lighting_from(lit), c.W, c.H, c.scale,
                              c.translation)
            check_frame(c.xyz, c.rgb, store, algo, c.W, c.H, c.scale, cam=cam, lit=lit, translation=c.translation,
                        gpu_scene=gpu, want=want)
        gpu.close()
        ref.close()


@pytest.mark.parametrize("name", ec.PICK_CASES)
def test_edge_picks(name):
    """vr.pick over every pixel against tests/pick_ref.py (held to the oracle on these cases by
    tests/test_edge_cases.py::test_pick_reference_agrees)."""
    c = ec.CASES[name]
    cam = gpu_camera(c)
    i = np.arange(c.W * c.H)
    px, py = (i % c.W).astype(np.uint32), (i // c.W).astype(np.uint32)
    info = vr.VoxelSceneInfo(c.translation, c.scale)
    for store in STORES:
        ps = pyref.Scene(c.xyz, c.rgb, int(store))
        with vr.create_scene(c.xyz, c.rgb, store) as scene:
            for algo in ALGOS:
                got = vr.pick(scene, algo, cam, info, c.W, c.H, px, py)
                with np.errstate(all="ignore"):
                    want, _ = pick_ref.pick_pixels(ps, cam, c.W, c.H, px, py, c.scale,
                                                   algo == vr.RayMarchAlgorithm.LONGEST_AXIS, c.translation)
                bad = pick_ref.same_records(got, want)
                assert bad.size == 0, (f"{store.name}/{algo.name}: {bad.size} of {len(got)} records differ; first at "
                                       f"pixel ({int(px[bad[0]])}, {int(py[bad[0]])}): gpu {got[bad[0]]} reference "
                                       f"{want[bad[0]]}")
                assert np.count_nonzero(got["status"] == vr.HitStatus.VOXEL) >= 32


def test_guards_are_reached():
    """One fresh child process renders every edge case, the alias fixture, one fuzz seed, two crawl views and the low-faces attempt once
    per store x algorithm through the counting build (the same sources with -DVR_DIAG), compares
    each frame with the oracle and reports the counters that moved.  Every counter of GUARDS moved
    in at least one of the cases named for it, or stands in UNREACHABLE with its argument (beside
    the site in vr_walk.h and in DESIGN.md section 4)."""
    assert os.path.exists(COVER_LIB), "libvr_cover.so is not built (make -C voxelraymarcher_amd/csrc)"
    env = dict(os.environ, VR_LIBRARY=COVER_LIB)
    p = subprocess.run([sys.executable, "-m", "tests.cover_run"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=240)
    assert p.returncode == 0, f"cover_run exited {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    rep = json.loads(p.stdout.strip().splitlines()[-1])
    assert rep["counters"] == 64
    assert not rep["differ"], f"frames of the counting build differ from the oracle: {rep['differ']}"
    assert rep["edge_cases"] == len(ec.CASES)
    assert {(r["case"], r["store"], r["algo"]) for r in rep["runs"]} >= {
        (n, vr.StorageType(s).name, vr.RayMarchAlgorithm(a).name) for n, s, a in ec.PAIRS}
    moved = {}                                      # counter -> {case: total}
    for run in rep["runs"]:
        for k, n in run["moved"].items():
            d = moved.setdefault(int(k), {})
            d[run["case"]] = d.get(run["case"], 0) + n
    for k in sorted(GUARDS):
        print(f"[{k:2d}] {GUARDS[k][0]:58s} {sum(moved.get(k, {}).values()):10d}  {sorted(moved.get(k, {}))}")
    missing = []
    for k, (what, cases) in GUARDS.items():
        if k in UNREACHABLE:
            assert not moved.get(k), f"counter {k} ({what}) is argued unreachable but moved: {moved[k]}"
            continue
        assert cases, f"counter {k} ({what}) names no case"
        if not any(moved.get(k, {}).get(c, 0) > 0 for c in cases):
            missing.append((k, what, cases, moved.get(k, {})))
    assert not missing, "guards not reached in their named cases: " + "; ".join(
        f"[{k}] {what}: expected in {cases}, moved in {got}" for k, what, cases, got in missing)
