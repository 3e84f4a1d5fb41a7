#!/usr/bin/env python3
"""Which HIP calls does each entry point that stages host or device arrays make?

Run mode calls vr_pick, vr_trace, vr_camera_rays, vr_scene_create_ex, vr_scene_edit and
vr_scene_voxels once in each staging mode on the golden scene (tests/golden/c1_scene.npz), through
ctypes on libvr.so (VR_LIBRARY selects another build) and on the HIP runtime for the device
buffers -- no torch, so a HIP API trace of the process holds the library's calls and this
script's only.  Every buffer is made before the first call; each call is preceded by one
hipRuntimeGetVersion, which nothing else here makes: the marker that cuts the trace into calls.
The labels of the calls, in order, go to the file named by --labels.

  rocprofv3 --hip-trace --output-format csv -d OUT -- python3 profiles/staging/api_sequence.py --labels OUT/labels.txt

Compare mode reads two such traces (the *_hip_api_trace.csv files) with their labels and prints
the ordered HIP API names of each call, once when the sides agree, both when they differ (calls
with the same sequences together, runs of one name as `name xN`):

  python3 profiles/staging/api_sequence.py --compare A.csv A_labels.txt B.csv B_labels.txt
"""
import csv
import ctypes
import os
import sys
from ctypes import byref, c_float, c_int, c_size_t, c_uint32, c_void_p

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
MARK = "hipRuntimeGetVersion"
SIZES = (1, 257)          # one lane; a second workgroup with one lane
W, H = 32, 24


def run(labels_path):
    import numpy as np

    try:
        hip = ctypes.CDLL("libamdhip64.so")
    except OSError:
        hip = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    vr = ctypes.CDLL(os.environ.get("VR_LIBRARY") or os.path.join(ROOT, "voxelraymarcher_amd", "libvr.so"))
    vr.vr_last_error.restype = ctypes.c_char_p
    labels = []

    def ok(rc, what):
        if rc:
            raise SystemExit(f"{what}: {rc} {vr.vr_last_error().decode() if what.startswith('vr_') else ''}")

    def dev(a):           # a device copy of a numpy array (made before the first marked call)
        p = c_void_p()
        ok(hip.hipMalloc(byref(p), c_size_t(max(a.nbytes, 16))), "hipMalloc")
        ok(hip.hipMemcpy(p, c_void_p(a.ctypes.data), c_size_t(a.nbytes), 1), "hipMemcpy")
        return p

    def host(a):
        return c_void_p(a.ctypes.data)

    def call(label, fn, *args):
        version = c_int()
        hip.hipRuntimeGetVersion(byref(version))
        ok(fn(*args), label)
        labels.append(label)

    d = np.load(os.path.join(ROOT, "tests", "golden", "c1_scene.npz"))
    xyz, rgb = np.ascontiguousarray(d["xyz"], np.int32), np.ascontiguousarray(d["rgb"], np.uint32)
    nvox = len(rgb)
    f3 = lambda *v: (c_float * 3)(*v)   # noqa: E731
    cam = (c_float * 15)()
    ok(vr.vr_camera_make(f3(6, 2, 6), f3(0, 0, -1), f3(0, 1, 0), c_float(60.0), c_float(W / H), cam), "vr_camera_make")
    tr = f3(0, 0, 0)
    scale = 12

    nmax = max(SIZES)
    i = np.arange(nmax) * 3 % (W * H)
    px, py = (i % W).astype(np.uint32), (i // W).astype(np.uint32)
    rays = np.zeros((nmax, 8), np.float32)
    hits = np.zeros((nmax, 16), np.uint32)
    out_xyz, out_rgb = np.zeros((nvox + 8, 3), np.int32), np.zeros(nvox + 8, np.uint32)
    # an edit: recolour the first 65 voxels, remove the next 64
    exyz = xyz[:129].copy()
    ergb = np.concatenate([np.full(65, 0x123456, np.uint32), np.full(64, 0xFFFFFFFF, np.uint32)])
    bufs = dict(px=dev(px), py=dev(py), rays=dev(rays), hits=dev(hits), xyz=dev(xyz), rgb=dev(rgb), exyz=dev(exyz),
                ergb=dev(ergb), out_xyz=dev(out_xyz), out_rgb=dev(out_rgb))
    ok(hip.hipDeviceSynchronize(), "hipDeviceSynchronize")
    modes = [(a, b) for a in (0, 1) for b in (0, 1)]
    io = lambda a, b: f"{'device' if a else 'host'} in, {'device' if b else 'host'} out"   # noqa: E731

    scenes = []
    for store in (0, 1):
        for on_dev in (0, 1):
            s = c_void_p()
            call(f"vr_scene_create_ex store {store}, {'device' if on_dev else 'host'} in", vr.vr_scene_create_ex, 0, store,
                 bufs["xyz"] if on_dev else host(xyz), bufs["rgb"] if on_dev else host(rgb), c_size_t(nvox), on_dev, 1,
                 None, byref(s))
            scenes.append((store, s))
    for store, s in scenes[1::2]:
        for n in SIZES:
            for a, b in modes:
                call(f"vr_camera_rays n {n}, {io(a, b)}", vr.vr_camera_rays, 0, cam, W, H, bufs["px"] if a else host(px),
                     bufs["py"] if a else host(py), c_size_t(n), a, bufs["rays"] if b else host(rays), b, None)
                call(f"vr_pick store {store} n {n}, {io(a, b)}", vr.vr_pick, s, 1, cam, tr, scale, W, H,
                     bufs["px"] if a else host(px), bufs["py"] if a else host(py), c_size_t(n), a,
                     bufs["hits"] if b else host(hits), b, None)
                for order in (1, 2):
                    call(f"vr_trace store {store} n {n} order {order}, {io(a, b)}", vr.vr_trace, s, 1, tr, scale,
                         bufs["rays"] if a else host(rays), c_size_t(n), a, bufs["hits"] if b else host(hits), b,
                         c_uint32(order), None)
        for on_dev in (0, 1):
            call(f"vr_scene_edit store {store}, {'device' if on_dev else 'host'} in", vr.vr_scene_edit, s,
                 bufs["exyz"] if on_dev else host(exyz), bufs["ergb"] if on_dev else host(ergb), c_size_t(len(ergb)), on_dev,
                 None)
            got = c_size_t()
            call(f"vr_scene_voxels store {store}, {'device' if on_dev else 'host'} out", vr.vr_scene_voxels, s,
                 bufs["out_xyz"] if on_dev else host(out_xyz), bufs["out_rgb"] if on_dev else host(out_rgb),
                 c_size_t(nvox + 8), on_dev, None, byref(got))
            assert 0 < got.value <= nvox, got.value
    call("(end: the script's own clean-up follows)", lambda: 0)
    vr.vr_scene_destroy.argtypes = [c_void_p]
    for _, s in scenes:
        vr.vr_scene_destroy(s)
    for p in bufs.values():
        hip.hipFree(p)
    assert np.count_nonzero(hits[:, 0] == 1) > 0 and np.isfinite(rays[:, :3]).all()
    with open(labels_path, "w") as f:
        f.write("\n".join(labels) + "\n")
    print(f"{len(labels) - 1} calls made")


def sequences(trace_csv, labels_path):
    rows = sorted(csv.DictReader(open(trace_csv)), key=lambda r: int(r["Start_Timestamp"]))
    labels = open(labels_path).read().splitlines()
    seqs, cur = [], None
    for r in rows:
        if r["Function"] == MARK:
            cur = []
            seqs.append(cur)
        elif cur is not None:
            cur.append(r["Function"])
    assert len(seqs) == len(labels), (len(seqs), len(labels))
    return labels[:-1], seqs[:-1]


LAUNCH = ["__hipPushCallConfiguration", "__hipPopCallConfiguration", "hipLaunchKernel"]


def short(seq):
    """The sequence in order, a kernel launch's three calls as `launch`, a run of one name as `name xN`."""
    names, i = [], 0
    while i < len(seq):
        if seq[i:i + 3] == LAUNCH:
            names.append("launch")
            i += 3
        else:
            names.append(seq[i])
            i += 1
    runs = []
    for n in names:
        if runs and runs[-1][0] == n:
            runs[-1][1] += 1
        else:
            runs.append([n, 1])
    return f"({len(seq)} calls) " + " ".join(n if k == 1 else f"{n} x{k}" for n, k in runs)


def compare(a_csv, a_labels, b_csv, b_labels):
    la, sa = sequences(a_csv, a_labels)
    lb, sb = sequences(b_csv, b_labels)
    assert la == lb
    print(f"launch = {' '.join(LAUNCH)}; calls that made the same sequences on both sides are listed together")
    groups = {}
    for label, x, y in zip(la, sa, sb):
        groups.setdefault((tuple(x), tuple(y)), []).append(label)
    differ = 0
    for (x, y), labels in groups.items():
        print("\n".join(labels))
        if x == y:
            print(f"  both {short(list(x))}")
        else:
            differ += len(labels)
            print(f"  DIFFER\n  a {short(list(x))}\n  b {short(list(y))}")
    print(f"{len(la)} entry-point calls, {differ} with a different HIP call sequence")
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) == 6 and sys.argv[1] == "--compare":
        sys.exit(compare(*sys.argv[2:]))
    if len(sys.argv) == 3 and sys.argv[1] == "--labels":
        sys.exit(run(sys.argv[2]))
    sys.exit(__doc__)
