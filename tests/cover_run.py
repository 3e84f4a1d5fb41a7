"""The child process of tests/test_gpu_edges.py::test_guards_are_reached: with VR_LIBRARY set to
the counting build (libvr_cover.so: the library's sources with -DVR_DIAG), render every edge
case (tests/edge_cases.py), the alias fixture, one fuzz seed, two crawl views
(tests/crawl_views.py: the crawl pass's generic loop) and the attempt on the site argued
unreachable (edge_cases.low_face_case) once per store x algorithm, compare each frame with the oracle, and print one JSON object -- per case and pair the
counters that moved (vr_diag_fetch, read and zeroed after each frame).

    VR_LIBRARY=voxelraymarcher_amd/libvr_cover.so python -m tests.cover_run

GUARDS names every counter index of the build: what it counts and the cases expected to move
it.  32 and up stand beside the rarely-taken blocks that keep the walks exact (vr_walk.h);
0-25 are the hot-loop counters of profiles/wave_counts.py, listed so that no index is without
an owner."""
from __future__ import annotations

import ctypes
import json
import os
import sys

N_COUNTERS = 64
ALIAS, FUZZ, LOW = "alias-fixture", "fuzz-1003", "low-faces"
CRAWL_PRIMARY, CRAWL_SHADOW = "crawl-y-plane", "crawl-shadow-x"     # tests/crawl_views.py, the cluster store
FUZZ_SEED = 1003

_TINY_DIR = ("E1-mixed", "E2-subnormal", "E3-two-tiny-2^-63", "E3-two-tiny-2^-124", "E7-pattern7-tiny")
_TINY_LIGHT = tuple(f"E4-light-{t}-{a}" for t in ("2^-70", "2^-130") for a in "xyz")
_SIGNS = ("E7-signs-ppp", "E7-signs-nnn")
_ANY = ("E1-mixed", "E5-far-origin", "E7-signs-ppp", FUZZ)

# index: (what the counter counts, the cases expected to move it)
GUARDS = {
    0: ("primary VCS walks (sign-specialised)", _ANY),
    1: ("primary VCS walks (generic loop: the crawl pass)", (CRAWL_PRIMARY,)),
    2: ("primary loop iterations (sign-specialised)", _ANY),
    3: ("primary loop iterations (generic loop)", (CRAWL_PRIMARY,)),
    4: ("shadow VCS walks (sign-specialised)", _ANY),
    5: ("shadow VCS walks (generic loop: the crawl pass)", (CRAWL_SHADOW,)),
    6: ("shadow loop iterations (sign-specialised)", _ANY),
    7: ("shadow loop iterations (generic loop)", (CRAWL_SHADOW,)),
    8: ("grid_original calls (primary)", _ANY),
    9: ("grid_original calls (shadow)", _ANY),
    10: ("primary region rounds", _ANY),
    11: ("primary null-region skips", (FUZZ,)),
    12: ("shadow region rounds", _ANY),
    13: ("shadow null-region skips", (FUZZ,)),
    14: ("primary() calls", _ANY),
    15: ("entry-clip iterations", ("E5-far-origin", "E6-tiny-numerator")),
    16: ("shadow walks started", _ANY),
    17: ("primary longest-axis walks", _ANY),
    18: ("primary longest-axis iterations", _ANY),
    19: ("shadow longest-axis walks", _ANY),
    20: ("shadow longest-axis iterations", _ANY),
    21: ("longest-axis iterations with a jumping lane", _ANY),
    22: ("primary iterations, no lane skipping", _ANY),
    23: ("primary iterations, every lane skipping", _ANY),
    24: ("shadow iterations, no lane skipping", _ANY),
    25: ("shadow iterations, every lane skipping", _ANY),
    32: ("initial step: IEEE fallback (direction or numerator outside the domain)", _TINY_DIR + _TINY_LIGHT),
    33: ("VCS walk, one divisor: IEEE fallback", ("E8-equal-tiny-light-pos",)),
    34: ("VCS walk, three divisors: IEEE fallback", _TINY_DIR + _TINY_LIGHT),
    35: ("cuckoo walk, one divisor: IEEE fallback", ("E8-equal-tiny-light-pos", "E8-equal-tiny-light-neg")),
    36: ("cuckoo walk, three divisors: IEEE fallback", _TINY_DIR + _TINY_LIGHT),
    37: ("longest-axis jump from a negative cell (C division form)", ()),
    38: ("longest-axis probe slot outside the region (aliasing form)", (ALIAS,)),
    39: ("entry clip: IEEE fallback", ("E5-far-origin", "E6-tiny-numerator")),
    # (the numerator image-plane point - eye must be below 2^-90: v * 2^-124, not v * 0.8 * 2^-63)
    40: ("ray direction: IEEE fallback (cuckoo store's ray generation)", ("E2-subnormal", "E3-two-tiny-2^-124")),
    41: ("a wave ran a second sign-pattern pass", _SIGNS + ("E1-mixed",)),
    42: ("pattern 7 through P,P,P: a lane's reciprocal outside the domain", ("E7-pattern7-tiny",) + _TINY_LIGHT),
    43: ("primary walks, sign pattern 0 (- - -)", ("E7-signs-nnn", LOW) + _TINY_LIGHT),
    44: ("primary walks, sign pattern 1 (+ - -)", _SIGNS),
    45: ("primary walks, sign pattern 2 (- + -)", _SIGNS + ("E1-mixed",)),
    46: ("primary walks, sign pattern 3 (+ + -)", _SIGNS + ("E7-pattern7-tiny",)),
    47: ("primary walks, sign pattern 4 (- - +)", _SIGNS),
    48: ("primary walks, sign pattern 5 (+ - +)", _SIGNS + ("E6-tiny-numerator",)),
    49: ("primary walks, sign pattern 6 (- + +)", _SIGNS + ("E1-mixed",)),
    50: ("primary walks, sign pattern 7 (+ + +)", ("E7-signs-ppp", "E7-pattern7-tiny", "E5-far-origin")),
    51: ("shadow walks, sign pattern 0 (- - -)", ("E5-far-origin",)),
    52: ("shadow walks, sign pattern 1 (+ - -)", ("E7-signs-ppp",)),
    53: ("shadow walks, sign pattern 2 (- + -)", ("E7-pattern7-tiny",)),
    54: ("shadow walks, sign pattern 3 (+ + -)", ("E2-subnormal", "E3-two-tiny-2^-124")),
    55: ("shadow walks, sign pattern 4 (- - +)", ("E7-signs-nnn",)),
    56: ("shadow walks, sign pattern 5 (+ - +)", ("E3-two-tiny-2^-63",)),
    57: ("shadow walks, sign pattern 6 (- + +)", ("E6-tiny-numerator",)),
    58: ("shadow walks, sign pattern 7 (+ + +)", ("E1-mixed",) + _TINY_LIGHT),
}
# index: where the argument that no finite input reaches it is written (and tried: LOW, ALIAS)
UNREACHABLE = {37: "vr_walk.h walk_longest_vcs, at the site; DESIGN.md section 4; "
                   "tests/test_edge_cases.py::test_no_jump_starts_in_a_negative_cell"}


def gpu_camera(c):
    """The vr.Camera of an edge case: the constructor's, or the raw fields written over one."""
    import voxelraymarcher_amd as vr
    from tests import edge_cases as ec
    if c.raw is None:
        return vr.Camera(c.eye, c.look_at, c.up, c.fov, c.aspect)
    cam = vr.Camera.reference(c.W, c.H)
    ec.set_raw(cam.raw, c)
    return cam


def gpu_lighting(c):
    import voxelraymarcher_amd as vr
    lit = vr.setup_constant_values(use_shadows=c.shadows, light_direction=c.light_dir, light_color=c.light_color)
    if c.raw_light is not None:                      # plain data: no makeUnitVector
        for i in range(3):
            lit.light_dir[i] = float(c.raw_light[i])
    return lit


def main() -> int:
    import numpy as np
    import torch

    import oracle
    import voxelraymarcher_amd as vr
    from tests import edge_cases as ec
    from tests import crawl_views as cv
    from tests.fuzz_cases import make_case
    from tests.helpers import GOLDEN, gpu_render, oracle_camera_from, oracle_lighting_from
    from voxelraymarcher_amd import _capi

    lib = _capi.lib()
    fetch = lib.vr_diag_fetch                      # only the counting build has it
    fetch.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]
    fetch.restype = ctypes.c_int
    buf = (ctypes.c_uint64 * N_COUNTERS)()

    # (name, voxels, camera, lighting, W, H, scale, translation, stores)
    views = []
    for name, c in ec.CASES.items():
        views.append((name, c.xyz, c.rgb, gpu_camera(c), gpu_lighting(c), c.W, c.H, c.scale, c.translation, c.stores))
    fx = json.load(open(os.path.join(GOLDEN, "alias_rays.json")))
    d = np.load(os.path.join(GOLDEN, fx["scene"]))
    n_edge = len(views)
    for k, cam in enumerate(fx["cameras"]):
        views.append((ALIAS, d["xyz"], d["rgb"], vr.Camera(cam["eye"], cam["at"], fx["up"], fx["fov"], fx["aspect"]),
                      vr.setup_constant_values(), fx["width"], fx["height"], 1, (0.0, 0.0, 0.0), (0, 1)))
    f = make_case(FUZZ_SEED)
    views.append((FUZZ, f.xyz, f.rgb, vr.Camera(f.eye, f.look_at, f.up, f.fov, f.aspect),
                  vr.setup_constant_values(use_shadows=f.shadows, use_point_light=f.point, light_position=f.light_pos,
                                           light_direction=f.light_dir, light_color=f.light_color),
                  f.W, f.H, f.scale, f.translation, (0, 1)))
    low = ec.low_face_case()
    views.append((LOW, low.xyz, low.rgb, gpu_camera(low), gpu_lighting(low), low.W, low.H, 1, low.translation, (0, 1)))
    for name, vname in ((CRAWL_PRIMARY, "y-plane"), (CRAWL_SHADOW, "shadow-x")):
        v = {w.name: w for w in cv.VIEWS}[vname]
        xyz, rgb = cv.SCENES[v.scene]()
        views.append((name, xyz, rgb, vr.Camera(v.world(v.eye), v.world(v.look_at), cv.UP, v.fov, cv.ASPECT),
                      vr.setup_constant_values(use_point_light=v.point, light_position=v.light_pos,
                                               light_direction=v.light_dir),
                      cv.W, cv.H, v.scale, v.translation, (0,)))

    assert fetch(buf, 1) == 0
    runs, differ = [], []
    for name, xyz, rgb, cam, lit, W, H, scale, tr, stores in views:
        info = vr.VoxelSceneInfo(tr, scale)
        for store in (vr.StorageType.VOXEL_CLUSTER_STORE, vr.StorageType.HASH_TABLE):
            if int(store) not in stores:
                continue
            ref = oracle.Scene(xyz, rgb, int(store))
            scene = vr.create_scene(xyz, rgb, store)
            for algo in (vr.RayMarchAlgorithm.ORIGINAL, vr.RayMarchAlgorithm.LONGEST_AXIS):
                want, _ = ref.render(int(algo), oracle_camera_from(cam), oracle_lighting_from(lit), W, H, scale, tr)
                got, _ = gpu_render(scene, algo, cam, lit, info, W, H)
                torch.cuda.synchronize()
                if fetch(buf, 1) != 0:
                    print("vr_diag_fetch failed", file=sys.stderr)
                    return 2
                bad = int(np.count_nonzero(got != want))
                if bad:
                    differ.append({"case": name, "store": store.name, "algo": algo.name, "pixels": bad})
                runs.append({"case": name, "store": store.name, "algo": algo.name,
                             "moved": {str(k): int(buf[k]) for k in range(N_COUNTERS) if buf[k]}})
            scene.close()
            ref.close()
    print(json.dumps({"counters": N_COUNTERS, "edge_cases": n_edge, "runs": runs, "differ": differ}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
