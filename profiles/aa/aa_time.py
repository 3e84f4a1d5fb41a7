"""What supersampled frames cost (profiles/aa/README.md), at 1920 x 1080 with S = 2 and 4
samples per axis:

    python profiles/aa/aa_time.py C2 C4 [--rounds 21]
    python profiles/aa/aa_time.py C2 C4 --render-only --root DIR    (the fine vr_render alone, with the
                    package of the built checkout at DIR -- the parent commit's; only calls it has)

Per config and S one JSON line with median / min / max in ms:

  (a) resolve / resolve_rgb8 / resolve_both / resolve_unaligned
                    vr_resolve alone on the fine frame (words, RGB8, both, and words from a fine buffer
                    4 bytes past a 16-byte boundary: the one-word loads), and memcpy_d2d: a
                    device-to-device hipMemcpyAsync of the fine frame's bytes.  A sample is one HIP
                    event pair around REPS back-to-back calls, divided by REPS; the calls are queued
                    behind a spinning kernel (torch.cuda._sleep), so the window holds no wait for
                    the host.  The same buffers every time: a 33 MB fine frame stays in the 256 MB
                    last-level cache between calls, as it does right after the render wrote it.
  (b) fine_first / aa_first        one vr_render of the fine frame / one vr_render_aa, each right after
                    vr_forget_orders (a first render of the view); a sample is one event pair around
                    one call.
      fine_repeat / aa_repeat      the same once the view's orders are learned (2 * slots + 2 warm-up
                    launches); a sample is one event pair around REPS calls on one stream, divided
                    by REPS.
  (c) torch_filter  what a caller did before: the box filter of the fine frame in torch (unpack the
                    channels, view(H, S, W, S), integer sum, round, repack), same words (checked
                    before timing: "same_words"); today_repeat = fine_repeat + torch_filter in one
                    window; torch_filter_peak_bytes: torch's peak allocation above the fine frame
                    during one filter.
The variants of a group alternate within each round, after WARM warm-up rounds."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if "--root" in sys.argv[1:-1]:       # (before the package is imported)
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)
import voxelraymarcher_amd as vr  # noqa: E402

WARM = 3
REPS = 10
SPIN_CYCLES = 4_000_000          # torch.cuda._sleep: about 2 ms, longer than the host needs to queue REPS calls
W, H = 1920, 1080


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def timed(fn, reps=1, behind=False):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    if behind:      # the calls queue up behind a spinning kernel, so the device never waits for the host
        torch.cuda._sleep(SPIN_CYCLES)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def hip_runtime():
    for name in ("libamdhip64.so.7", "libamdhip64.so"):
        try:
            return ctypes.CDLL(name)
        except OSError:
            continue
    raise OSError("the HIP runtime torch loaded was not found by name")


def torch_filter(fine, S):
    """The caller's own box filter: the resolved words of a (S * H, S * W) int32 tensor."""
    n, shift = S * S, 2 * (S.bit_length() - 1)
    f = fine.view(H, S, W, S)
    out = None
    for sh in (16, 8, 0):
        c = (((f >> sh) & 0xFF).sum(dim=(1, 3), dtype=torch.int32) + n // 2) >> shift
        out = c << sh if out is None else out | (c << sh)
    return out


def rounds_of(calls, rounds, reps, behind=False):
    samples = {k: [] for k in calls}
    for r in range(WARM + rounds):
        for k, fn in calls.items():
            ms = timed(fn, reps, behind)
            if r >= WARM:
                samples[k].append(ms)
    return {k: stats(v) for k, v in samples.items()}


def measure(name: str, S: int, rounds: int, render_only: bool):
    cfg = vr.CONFIGS[name]
    xyz, rgb = cfg.voxels()
    scene = vr.create_scene(xyz, rgb, cfg.store)
    del xyz, rgb
    cam, lit = vr.Camera.reference(W, H), vr.setup_constant_values()
    info = vr.VoxelSceneInfo((0.0, 0.0, 0.0), cfg.scale)
    fw, fh = S * W, S * H
    fine = torch.empty(fw * fh, dtype=torch.int32, device="cuda")
    slots = vr.debug_order_uses(0)["slots"]
    res = {"config": name, "samples": S, "fine": [fw, fh], "rounds": rounds, "reps": REPS, "slots": slots,
           "library": os.path.relpath(vr.LIB_PATH)}

    def fine_render():
        vr.run_raymarching_kernel(scene, cfg.algorithm, cam, lit, info, fw, fh, out=fine)

    def first(fn):
        def run():
            vr.forget_orders(0)
            return timed(fn)
        return run

    if render_only:
        res["fine_first"] = stats([first(fine_render)() for _ in range(WARM + rounds)][WARM:])
        for _ in range(2 * slots + 2):
            fine_render()
        res.update(rounds_of({"fine_repeat": fine_render}, rounds, REPS))
        print(json.dumps(res), flush=True)
        scene.close()
        return

    out = torch.empty(H * W, dtype=torch.int32, device="cuda")
    rgb8 = torch.empty(H * W * 3, dtype=torch.uint8, device="cuda")

    def aa():
        vr.render_aa(scene, cfg.algorithm, cam, lit, info, W, H, S, fine=fine, out=out)

    # the words first: vr_render_aa, vr_resolve of the fine render and the torch filter agree
    aa()
    torch.cuda.synchronize()
    got = out.clone()
    fine_render()
    res["same_words"] = bool(torch.equal(vr.resolve(fine, W, H, S).view(-1), got)) and \
        bool(torch.equal(torch_filter(fine, S).view(-1), got))
    res["changed_pixels"] = int((got != vr.run_raymarching_kernel(scene, cfg.algorithm, cam, lit, info, W, H)).sum())

    # (a) the filter alone against a device-to-device copy of the same bytes
    hip = hip_runtime()
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipMemcpyAsync.restype = ctypes.c_int
    copy = torch.empty_like(fine)
    shifted = torch.empty(fine.numel() + 1, dtype=torch.int32, device="cuda")[1:]
    shifted.copy_(fine)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def memcpy():
        rc = hip.hipMemcpyAsync(copy.data_ptr(), fine.data_ptr(), fine.numel() * 4, 3, stream)   # 3: device to device
        assert rc == 0, rc

    def resolve_call(src, words, rgb):      # vr_resolve itself, its arguments made once
        fn, args = vr.lib().vr_resolve, (ctypes.c_void_p(src.data_ptr()), W, H, S,
                                         ctypes.c_void_p(words.data_ptr()) if words is not None else None,
                                         ctypes.c_void_p(rgb.data_ptr()) if rgb is not None else None, stream)

        def call():
            rc = fn(*args)
            assert rc == 0, rc
        return call

    res.update(rounds_of({
        "resolve": resolve_call(fine, out, None),
        "resolve_rgb8": resolve_call(fine, None, rgb8),
        "resolve_both": resolve_call(fine, out, rgb8),
        "resolve_unaligned": resolve_call(shifted, out, None),
        "memcpy_d2d": memcpy}, rounds, REPS, behind=True))
    assert torch.equal(copy, fine)
    res["resolve_over_memcpy"] = round(res["resolve"]["median_ms"] / res["memcpy_d2d"]["median_ms"], 3)
    res["fine_bytes"] = fine.numel() * 4

    # (b) per frame: a first render of the view, alternating
    first_calls = {"fine_first": first(fine_render), "aa_first": first(aa)}
    first_s = {k: [] for k in first_calls}
    for r in range(WARM + rounds):
        for k, fn in first_calls.items():
            ms = fn()
            if r >= WARM:
                first_s[k].append(ms)
    res.update({k: stats(v) for k, v in first_s.items()})

    # (b), (c) the repeated view: each variant warmed until its view is under its orders (the two
    # render the same fine view, so they share them)
    for _ in range(2 * slots + 2):
        aa()

    def today():
        fine_render()
        return torch_filter(fine, S)

    res.update(rounds_of({"fine_repeat": fine_render, "aa_repeat": aa, "torch_filter": lambda: torch_filter(fine, S),
                          "today_repeat": today}, rounds, REPS))
    res["aa_minus_fine_repeat_ms"] = round(res["aa_repeat"]["median_ms"] - res["fine_repeat"]["median_ms"], 4)
    res["aa_minus_fine_first_ms"] = round(res["aa_first"]["median_ms"] - res["fine_first"]["median_ms"], 4)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    keep = torch_filter(fine, S)
    torch.cuda.synchronize()
    res["torch_filter_peak_bytes"] = int(torch.cuda.max_memory_allocated() - base)
    res["resolved_bytes"] = keep.numel() * 4
    print(json.dumps(res), flush=True)
    scene.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="+")
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--samples", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--render-only", action="store_true")
    ap.add_argument("--root", help="the built checkout whose package to measure (default: this one)")
    args = ap.parse_args()
    assert args.rounds >= 7 and torch.cuda.is_available(), "needs a GPU"
    for name in args.configs:
        for S in args.samples:
            measure(name, S, args.rounds, args.render_only)
