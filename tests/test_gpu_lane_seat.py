"""GPU test of the lane order's seats (vr_order.hip perm_kernel, vr_march.hip lane_pixel): a repeated view
learns, per pixel block, which 64 pixels each wave slot renders (the cost-rank deal) and in
which lane of the slot each pixel sits (VR_LANE_SEAT: cost order or ascending Morton order of
the pixel's column and row in the block).  The order is read back through
vr_debug_lane_order together with the walk lengths it was made from, so the deal is checked
against the same rule in numpy, for whichever block shape and seat rule the library was built
with.  Frames: full blocks only (32x32), full blocks plus blocks cut at both edges (48x40),
and a frame that holds full blocks of every shape up to 32x32 (64x32)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import oracle
from tests.order_model import morton

pytestmark = pytest.mark.gpu

vr = pytest.importorskip("voxelraymarcher_amd")

FRAMES = [(32, 32), (48, 40), (64, 32)]
LAUNCHES = 40          # past two uses of each of the ring's 16 slots: every slot learns and reuses


@pytest.mark.parametrize("size", FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("store", ["vcs", "hashtable"])
def test_lane_seats(store, size):
    W, H = size
    cfg = vr.CONFIGS["C1"]
    xyz, rgb = cfg.voxels()
    st = vr.parse_storage(store)
    scene = vr.create_scene(xyz, rgb, st)
    algo = vr.RayMarchAlgorithm.ORIGINAL
    cam, lit = vr.Camera.reference(W, H), vr.setup_constant_values()
    info = vr.VoxelSceneInfo((0.0, 0.0, 0.0), cfg.scale)
    dev = torch.cuda.current_device()
    vr.forget_orders(dev)
    vr.debug_capture_lane_order(dev)

    # (a) every frame of the repeated view, before and after the orders are learned, is the
    # first render word for word, and that is the oracle's frame
    first = None
    for i in range(LAUNCHES):
        out = torch.full((W * H,), -1, dtype=torch.int32, device="cuda")
        vr.run_raymarching_kernel(scene, algo, cam, lit, info, W, H, out)
        torch.cuda.synchronize()
        if first is None:
            first = out.clone()
        assert torch.equal(out, first), (store, W, H, i)
    ref = oracle.Scene(xyz, rgb, int(st))
    want, _ = ref.render(int(algo), oracle.reference_camera(W, H), oracle.lighting(), W, H, cfg.scale)
    ref.close()
    got = first.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, np.asarray(want).reshape(-1)), (store, W, H)

    shape, pcost, perm = vr.debug_lane_order(dev)
    scene.close()
    assert (shape["LW"], shape["rows"]) == (W, H)
    X, Y, seat = shape["block_x"], shape["block_y"], shape["seat"]
    n = X * Y
    shift = n.bit_length() - 1
    gx, gy = shape["gx"], shape["gy"]
    kx, ky = X // 16, Y // 8                      # tile groups (16x8 pixels) per block side
    nbx, nby = -(-gx // kx), -(-gy // ky)
    assert perm.shape == (nbx * nby, n)
    assert len(np.unique(pcost)) > 1, "the view's walk lengths are all equal: nothing to order"
    # the walk lengths of the padded grid (a full block may reach past the frame: zeros there)
    pad = np.zeros((nby * Y, nbx * X), dtype=np.uint32)
    pad[:H, :W] = pcost
    t = np.arange(n, dtype=np.uint32)
    code = morton(t % X, t // X)
    full = 0
    for BY in range(nby):
        for BX in range(nbx):
            if (BX + 1) * kx > gx or (BY + 1) * ky > gy:
                continue                          # cut by the grid's edge: 8x8 tiles, perm unused
            full += 1
            got_perm = perm[BY * nbx + BX].astype(np.uint32)
            # (b) a permutation of the block's pixels
            assert np.array_equal(np.sort(got_perm), t), (BX, BY)
            w = pad[BY * Y:(BY + 1) * Y, BX * X:(BX + 1) * X].reshape(-1)
            p, s = w >> 16, w & 0xFFFF
            c = np.minimum(np.maximum(p, s) + ((p + s) >> 3), (1 << (32 - shift)) - 1).astype(np.uint32)
            ranked = np.sort(c << shift | t)[::-1] & (n - 1)      # heaviest first, distinct keys
            for q in range(n // 64):
                slot = got_perm[64 * q:64 * q + 64]
                # (c) the slot's pixels are ranks 64 q .. 64 q + 63 of the cost order
                assert np.array_equal(np.sort(slot), np.sort(ranked[64 * q:64 * q + 64])), (BX, BY, q)
                # (d) seated by the build's rule
                if seat == 1:
                    assert np.all(np.diff(code[slot].astype(np.int64)) > 0), (BX, BY, q)
                else:
                    assert np.array_equal(slot, ranked[64 * q:64 * q + 64]), (BX, BY, q)
    assert full >= 1
