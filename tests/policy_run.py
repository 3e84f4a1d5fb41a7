"""The child process of tests/test_gpu_crawl_width.py and tests/test_gpu_in_flight_policy.py:
render a set of small cases under the launch-policy knobs of the environment it was started
with, compare every launch with the live oracle, and print one JSON line.

    VR_CRAWL_RPW=33 python -m tests.policy_run width
    VR_ORDER_REFRESH=1 python -m tests.policy_run knobs [--in-flight]

The knobs (vr_launch.cpp policy_knobs, order_refresh, crawl_skip_enabled) are function-local
statics read once per process, so only a fresh process can run under another value; the parent
starts one child at a time through subprocess.run(..., env=...).  The child proves which policy
its launches got from vr_debug_last_launch, never from its environment: Launches wraps the
package's two render entry points and reads the hook after every launch.

Case set `width` (the crawl pass at one records-per-wave width):
  * the NaN-camera frame of test_never_ending_walks at 64x64 (most of 4096 pixels defer) and
    the degenerate-light frame of test_degenerate_light_direction at 96x96, both stores, both
    algorithms, defer_caps (0, 16);
  * every view of tests/crawl_views.py at 48x32 on the cluster store, both algorithms, kernels
    TILE and TILE_REWALK, defer_caps (0, 4).
  Per case, kernel and capacity: one counted launch with `stats` (pixels, algorithmic bytes, the
  hook's values, the stats pair), then check_frame (tests/test_gpu_parity.py) with every one of
  its assertions.  The cluster store's NaN frame comes first: a child's first launch has the
  64-workgroup crawl grid (no hint yet) and thousands of records.

Case set `knobs` (knob branches no other test enters): fuzz seed 1000 (both stores) and the
crawl view x-plane, both algorithms, each through render_learned (tests/helpers.py) with the
order counters read after every launch; --in-flight turns vr_debug_force_in_flight on first.

A wrong frame is a reported mismatch (exit 1), never an exception that loses the report; an
error of the library ends the run at that case (exit 2) with the report so far."""
from __future__ import annotations

import json
import sys
import time

PLAN = ("alone", "heavy", "hi", "crawl_rpw")
NAN_FRAME, DEGENERATE = "nan-camera", "degenerate-light"


class Launches:
    """While entered, every vr.render_ex / vr.run_raymarching_kernel call is followed by a read
    of vr_debug_last_launch and vr_debug_order_uses (host state only): `plans` counts the
    (alone, heavy, hi, crawl_rpw) tuples seen, `skipped` the launches whose crawl pass did not
    run, `grids` the crawl grids, `orders` the (lane_orders_made, work_orders_made,
    lane_order_uses, work_order_uses, crawl_skips) counters after each launch."""

    def __init__(self, device=0):
        self.device = device
        self.reset()

    def reset(self):
        self.n, self.skipped, self.plans, self.grids, self.orders = 0, 0, {}, set(), []

    def note(self):
        import voxelraymarcher_amd as vr
        d = vr.debug_last_launch(self.device)
        u = vr.debug_order_uses(self.device)
        self.n += 1
        self.skipped += not d["crawl_ran"]
        key = tuple(d[k] for k in PLAN)
        self.plans[key] = self.plans.get(key, 0) + 1
        self.grids.add(d["crawl_grid"])
        self.orders.append([u["lane_orders_made"], u["work_orders_made"], u["lane_order_uses"], u["work_order_uses"],
                            u["crawl_skips"]])

    def __enter__(self):
        import voxelraymarcher_amd as vr
        self.saved = (vr.render_ex, vr.run_raymarching_kernel)

        def wrap(fn):
            def call(*a, **k):
                r = fn(*a, **k)
                self.note()
                return r
            return call
        vr.render_ex, vr.run_raymarching_kernel = wrap(self.saved[0]), wrap(self.saved[1])
        return self

    def __exit__(self, *exc):
        import voxelraymarcher_amd as vr
        vr.render_ex, vr.run_raymarching_kernel = self.saved
        return False

    def report(self) -> dict:
        return {"launches": self.n, "crawl_not_run": self.skipped, "grids": sorted(self.grids),
                "plans": [list(k) + [c] for k, c in sorted(self.plans.items())]}


def nan_case():
    """test_never_ending_walks' frame: (voxels, vr.Camera, oracle camera, lighting, W, H, scale)."""
    import voxelraymarcher_amd as vr
    from tests.test_oracle import nan_camera
    xyz, rgb = vr.CONFIGS["C1"].voxels()
    cam = vr.Camera.reference(64, 64)
    for f in ("origin", "lower_left"):
        for i in range(3):
            getattr(cam.raw, f)[i] = 1.0
    for f in ("horizontal", "vertical", "forward"):
        for i in range(3):
            getattr(cam.raw, f)[i] = 0.0
    return xyz, rgb, cam, nan_camera(), vr.setup_constant_values(), 64, 64, 12


def degenerate_light_case():
    """test_degenerate_light_direction's frame: light direction and colour written as plain data."""
    import voxelraymarcher_amd as vr
    from tests.helpers import oracle_camera_from
    xyz, rgb = vr.CONFIGS["C1"].voxels()
    lit = vr.setup_constant_values()
    for i in range(3):
        lit.light_dir[i] = 1e-6
        lit.light_color[i] = 1e6
    cam = vr.Camera.reference(96, 96)
    return xyz, rgb, cam, oracle_camera_from(cam), lit, 96, 96, vr.CONFIGS["C1"].scale


def crawl_view_case(view):
    """A view of tests/crawl_views.py: (voxels, vr.Camera, oracle camera, lighting, W, H, scale)."""
    import voxelraymarcher_amd as vr
    from tests import crawl_views as cv
    from tests.helpers import oracle_camera_from
    xyz, rgb = cv.SCENES[view.scene]()
    cam = vr.Camera(view.world(view.eye), view.world(view.look_at), cv.UP, view.fov, cv.ASPECT)
    lit = vr.setup_constant_values(use_point_light=view.point, light_position=view.light_pos,
                                   light_direction=view.light_dir)
    return xyz, rgb, cam, oracle_camera_from(cam), lit, cv.W, cv.H, view.scale


def fuzz_case(seed):
    import voxelraymarcher_amd as vr
    from tests.fuzz_cases import make_case, make_wide_case
    from tests.helpers import oracle_camera_from
    c = make_wide_case(seed) if seed >= 5000 else make_case(seed)
    cam = vr.Camera(c.eye, c.look_at, c.up, c.fov, c.aspect)
    lit = vr.setup_constant_values(use_shadows=c.shadows, use_point_light=c.point, light_position=c.light_pos,
                                   light_direction=c.light_dir, light_color=c.light_color)
    return c.xyz, c.rgb, cam, oracle_camera_from(cam), lit, c.W, c.H, c.scale, c.translation


def width_cases():
    """(name, case tuple, translation, stores, kernels, defer_caps); the cluster store's NaN frame first."""
    import voxelraymarcher_amd as vr
    from tests import crawl_views as cv
    tile, both = [vr.Kernel.TILE], [vr.Kernel.TILE, vr.Kernel.TILE_REWALK]
    zero = (0.0, 0.0, 0.0)
    yield NAN_FRAME, nan_case(), zero, (0, 1), tile, (0, 16)
    for v in cv.VIEWS:
        yield "crawl-" + v.name, crawl_view_case(v), v.translation, (0,), both, (0, 4)
    yield DEGENERATE, degenerate_light_case(), zero, (0, 1), tile, (0, 16)


def run_width(log, report):
    import numpy as np
    import torch

    import oracle
    import voxelraymarcher_amd as vr
    from tests.helpers import diff_report, oracle_lighting_from
    from tests.test_gpu_parity import check_frame

    for name, (xyz, rgb, cam, ocam, lit, W, H, scale), tr, stores, kernels, caps in width_cases():
        info = vr.VoxelSceneInfo(tr, scale)
        for store in stores:
            ref = oracle.Scene(xyz, rgb, store)
            scene = vr.create_scene(xyz, rgb, vr.StorageType(store))
            for algo in (vr.RayMarchAlgorithm.ORIGINAL, vr.RayMarchAlgorithm.LONGEST_AXIS):
                want = ref.render(int(algo), ocam, oracle_lighting_from(lit), W, H, scale, tr)
                for kernel in kernels:
                    for cap in caps:
                        t0 = time.perf_counter()
                        log.reset()
                        out = torch.full((W * H,), -1, dtype=torch.int32, device="cuda")
                        ctr = torch.zeros(1, dtype=torch.int64, device="cuda")
                        st = torch.zeros(2, dtype=torch.int64, device="cuda")
                        vr.render_ex(scene, algo, cam, lit, info, W, H, out, counter=ctr, stats=st, kernel=kernel,
                                     defer_cap=cap)
                        torch.cuda.synchronize()
                        first = vr.debug_last_launch(log.device)
                        got, nbytes = out.cpu().numpy().view(np.uint32), int(ctr.item())
                        bad = None
                        if not np.array_equal(got, want[0]):
                            bad = "first launch: " + diff_report(got, want[0], W)
                        elif nbytes != want[1]:
                            bad = f"first launch: algorithmic bytes: gpu {nbytes} != oracle {want[1]}"
                        try:
                            check_frame(xyz, rgb, vr.StorageType(store), algo, W, H, scale, cam=cam, lit=lit,
                                        translation=tr, gpu_scene=scene, want=want, kernels=[kernel], defer_caps=(cap,))
                        except AssertionError as e:
                            bad = bad or str(e)
                        run = {"case": name, "store": int(store), "algo": algo.name, "kernel": kernel.name,
                               "defer_cap": cap, "first": first, "stats": [int(x) for x in st.tolist()],
                               "mismatch": bad, "seconds": round(time.perf_counter() - t0, 3)}
                        run.update(log.report())
                        report["runs"].append(run)
            scene.close()
            ref.close()


def run_knobs(log, report):
    import oracle
    import voxelraymarcher_amd as vr
    from tests import crawl_views as cv
    from tests.helpers import diff_report, oracle_lighting_from, render_learned

    xplane = {v.name: v for v in cv.VIEWS}["x-plane"]
    cases = [("fuzz-1000", fuzz_case(1000), (0, 1)),
             ("crawl-x-plane", crawl_view_case(xplane) + (xplane.translation,), (0,))]
    for name, (xyz, rgb, cam, ocam, lit, W, H, scale, tr), stores in cases:
        info = vr.VoxelSceneInfo(tr, scale)
        for store in stores:
            ref = oracle.Scene(xyz, rgb, store)
            scene = vr.create_scene(xyz, rgb, vr.StorageType(store))
            for algo in (vr.RayMarchAlgorithm.ORIGINAL, vr.RayMarchAlgorithm.LONGEST_AXIS):
                want = ref.render(int(algo), ocam, oracle_lighting_from(lit), W, H, scale, tr)[0]
                t0 = time.perf_counter()
                log.reset()
                before = vr.debug_order_uses(log.device)
                bad, first, d = render_learned(scene, algo, cam, lit, info, W, H, 0, H, want, None, 0)
                run = {"case": name, "store": int(store), "algo": algo.name, "delta": d,
                       "records": vr.debug_last_launch(log.device)["records"],
                       "before": [before[k] for k in ("lane_orders_made", "work_orders_made", "lane_order_uses",
                                                      "work_order_uses", "crawl_skips")],
                       "orders": log.orders,
                       "mismatch": f"launches {bad} differ: " + diff_report(first, want, W) if bad else None,
                       "seconds": round(time.perf_counter() - t0, 3)}
                run.update(log.report())
                report["runs"].append(run)
            scene.close()
            ref.close()


KNOBS = ("VR_ORDER_REFRESH", "VR_ORDER", "VR_LANE_ORDER", "VR_CRAWL_SKIP", "VR_INFLIGHT_HEAVY", "VR_INFLIGHT_WAVES",
         "VR_CRAWL_RPW", "VR_CRAWL_RPW_IN_FLIGHT")
STOP_CODES = (134, 139, 124, 137)      # abort, segmentation fault, time limits
CHILD_TIMEOUT = 240                    # seconds: tests/test_gpu_edges.py's bound for cover_run


def run_child(caseset, knobs, in_flight=False):
    """The parent's side: one child with exactly the knobs given (any the parent inherited are
    dropped), waited for.  Returns (report, stop, seconds): `report` the child's JSON line (None
    when it left none), `stop` None or why no further child may be started -- the child ended
    by a signal, with one of STOP_CODES, at the timeout, or with anything but 0 (frames equal)
    or 1 (mismatches reported), which is how it ends after an error of the library."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update({k: str(v) for k, v in knobs.items()})
    cmd = [sys.executable, "-m", "tests.policy_run", caseset] + (["--in-flight"] if in_flight else [])
    t0 = time.perf_counter()
    try:
        p = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        left = (e.stdout or b"")[-2000:], (e.stderr or b"")[-4000:]
        return None, f"{knobs}: no answer in {CHILD_TIMEOUT} s; it left:\n{left[0]!r}\n{left[1]!r}", CHILD_TIMEOUT
    seconds = time.perf_counter() - t0
    report = None
    lines = p.stdout.strip().splitlines()
    if lines and lines[-1].startswith("{"):
        try:
            report = json.loads(lines[-1])
        except ValueError:
            pass
    stop = None
    if p.returncode not in (0, 1) or report is None:
        how = "a signal" if p.returncode < 0 else ("a stop code" if p.returncode in STOP_CODES else "an error")
        stop = (f"{knobs}: the child ended with {p.returncode} ({how}); it left:\n{p.stdout[-2000:]}\n"
                f"{p.stderr[-4000:]}")
    return report, stop, seconds


def main(argv) -> int:
    caseset = argv[1] if len(argv) > 1 else ""
    if caseset not in ("width", "knobs"):
        print("usage: python -m tests.policy_run width|knobs [--in-flight]", file=sys.stderr)
        return 2
    import traceback

    import voxelraymarcher_amd as vr
    report = {"caseset": caseset, "in_flight": "--in-flight" in argv[2:], "runs": [], "error": None}
    log = Launches(0)
    t0 = time.perf_counter()
    try:
        vr.debug_force_in_flight(log.device, report["in_flight"])
        with log:
            (run_width if caseset == "width" else run_knobs)(log, report)
    except Exception:       # an error of the library (a HIP error included): nothing more is launched
        report["error"] = traceback.format_exc()[-2000:]
    report["seconds"] = round(time.perf_counter() - t0, 3)
    print(json.dumps(report))
    sys.stdout.flush()
    if report["error"]:
        return 2
    return 1 if any(r["mismatch"] for r in report["runs"]) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
