"""Shared helpers: render one configuration through the HIP path (C ABI) and
through the CPU oracle with identical inputs."""
from __future__ import annotations

import os

import numpy as np

import oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def oracle_camera_from(cam) -> "oracle.OrCamera":
    """Copy a vr.Camera's fields into the oracle struct (same host math, checked separately)."""
    c = oracle.OrCamera()
    for f in ("origin", "lower_left", "horizontal", "vertical", "forward"):
        for i in range(3):
            getattr(c, f)[i] = getattr(cam.raw, f)[i]
    return c


def oracle_lighting_from(lit) -> "oracle.OrLighting":
    o = oracle.OrLighting()
    for f in ("light_dir", "light_color", "light_pos"):
        for i in range(3):
            getattr(o, f)[i] = getattr(lit, f)[i]
    o.use_point_light = lit.use_point_light
    o.use_shadows = lit.use_shadows
    return o


def gpu_render(scene, algo, cam, lit, info, W, H, row_begin=0, row_end=None, count=False, kernel=None, defer_cap=0):
    import torch

    import voxelraymarcher_amd as vr
    row_end = H if row_end is None else row_end
    kernel = vr.Kernel.AUTO if kernel is None else kernel
    out = torch.full(((row_end - row_begin) * W,), -1, dtype=torch.int32, device="cuda")
    nbytes = None
    if count or defer_cap:
        ctr = torch.zeros(1, dtype=torch.int64, device="cuda") if count else None
        vr.render_ex(scene, algo, cam, lit, info, W, H, out, row_begin, row_end, counter=ctr, kernel=kernel,
                     defer_cap=defer_cap)
        torch.cuda.synchronize()
        nbytes = int(ctr.item()) if count else None
    else:
        vr.run_raymarching_kernel(scene, algo, cam, lit, info, W, H, out, row_begin, row_end, kernel=kernel)
        torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32), nbytes


def differing_launches(frames, want):
    """The comparison of render_learned: `frames` yields one tensor per launch (it may be the
    same buffer each time), `want` is a tensor on the same device.  Returns the indices of the
    launches whose frame is not `want` (torch.equal, on the frames' device) and the first such
    frame as a host uint32 array (None when all agree), for diff_report."""
    import torch
    bad, first = [], None
    for k, frame in enumerate(frames):
        if not torch.equal(frame, want):
            bad.append(k)
            if first is None:
                first = frame.cpu().numpy().view(np.uint32).copy()
    return bad, first


ORDER_COUNTERS = ("launches", "lane_orders_made", "lane_order_uses", "work_orders_made", "work_order_uses",
                  "crawl_skips")


def render_learned(scene, algo, cam, lit, info, W, H, row_begin, row_end, want, kernel, defer_cap, schedule=None,
                   launches=None, out=None, **deal):
    """The uncounted view launched `launches` times in a row on the current stream -- by
    default 2 * slots + 2 with the slot count of vr_debug_order_uses: launch k takes slot
    k mod slots, launches 1..slots all repeat the view, so each slot either holds the view's
    orders already or makes them, and launches slots + 1 .. 2 slots + 1 (at least slots + 1
    of them, every slot at least once) render under them.  Every launch goes into a buffer
    refilled with -1, is waited for and compared on the device with `want` (the oracle's
    pixels as a uint32 array, or an int32 tensor on the device).  `deal`: render_ex's
    band_rows / rank / nranks / tile_cols / deal_stride; `out`: the buffer to render into (it
    keeps the last launch).  Returns (indices of the launches that differ, the first
    differing frame as a host array, the rise of each vr_debug_order_uses counter plus
    "slots" and "lane_block")."""
    import torch

    import voxelraymarcher_amd as vr
    row_end = H if row_end is None else row_end
    kernel = vr.Kernel.AUTO if kernel is None else kernel
    schedule = vr.Schedule.AUTO if schedule is None else schedule
    device = scene.info()["device"]
    before = vr.debug_order_uses(device)
    launches = 2 * before["slots"] + 2 if launches is None else launches
    rows, band = row_end - row_begin, deal.get("band_rows", 0) or max(1, row_end - row_begin)
    if deal.get("tile_cols"):
        words = vr.tile_buffer_words(W, rows, band, deal["tile_cols"], deal.get("nranks", 1))
    else:
        words = vr.band_buffer_words(W, rows, band, deal.get("nranks", 1))
    if not torch.is_tensor(want):
        want = torch.from_numpy(np.ascontiguousarray(want).view(np.int32)).to(f"cuda:{device}")
    assert want.numel() == words, (want.numel(), words)
    out = torch.empty(words, dtype=torch.int32, device=want.device) if out is None else out

    def frames():
        for _ in range(launches):
            out.fill_(-1)
            vr.render_ex(scene, algo, cam, lit, info, W, H, out, row_begin, row_end, kernel=kernel,
                         defer_cap=defer_cap, schedule=schedule, **deal)
            torch.cuda.synchronize(want.device)
            yield out

    bad, first = differing_launches(frames(), want)
    after = vr.debug_order_uses(device)
    delta = {k: after[k] - before[k] for k in ORDER_COUNTERS}
    delta["slots"], delta["lane_block"] = after["slots"], after["lane_block"]
    assert delta["launches"] == launches, delta
    return bad, first, delta


def full_lane_blocks(W, rows, lane_block) -> int:
    """How many whole lane blocks (vr_debug_order_uses' lane_block, pixels) the tile pass's grid
    of 16x8-pixel tile groups holds for a W x rows buffer: only those deal their pixels by the
    lane order, blocks cut by the grid's edge keep the 8x8 tiles."""
    lbx, lby = lane_block[0] // 16, lane_block[1] // 8
    return (-(-W // 16) // lbx) * (-(-rows // 8) // lby)


def diff_report(got: np.ndarray, want: np.ndarray, W: int, row_begin: int = 0) -> str:
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return "identical"
    lines = [f"{bad.size} of {got.size} pixels differ"]
    for i in bad[:8]:
        lines.append(f"  (x={i % W}, y={row_begin + i // W}): gpu=0x{int(got[i]):08x} oracle=0x{int(want[i]):08x}")
    return "\n".join(lines)
