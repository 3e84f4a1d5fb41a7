"""The tile pass's per-ray sign dispatch against the oracle: views whose 8 x 8 tiles hold several
direction-sign patterns, whose rays cross different numbers of regions and meet an empty region
(tests/sign_dispatch_cases.py; tests/test_sign_dispatch_cases.py asserts those preconditions on
the CPU).  Every case is held to the oracle by tests/test_gpu_parity.check_frame: pixels and
counted bytes bit for bit, counted and uncounted launches, and relaunches under the learned lane
and work orders -- on both stores.  On the cluster store the pick and trace kernels, which keep
the one generic loop, must describe the same hits."""
from __future__ import annotations

import numpy as np
import pytest

import oracle
from tests import pick_ref, pyref
from tests import sign_dispatch_cases as sd
from tests.cover_run import gpu_camera, gpu_lighting
from tests.helpers import diff_report, oracle_camera_from, oracle_lighting_from
from tests.test_edge_cases import pyref_lighting
from tests.test_gpu_parity import check_frame

pytestmark = pytest.mark.gpu

vr = pytest.importorskip("voxelraymarcher_amd")
torch = pytest.importorskip("torch")

VCS, HASH = vr.StorageType.VOXEL_CLUSTER_STORE, vr.StorageType.HASH_TABLE
ORIGINAL = vr.RayMarchAlgorithm.ORIGINAL
W, H = sd.W, sd.H
INFO = vr.VoxelSceneInfo((0.0, 0.0, 0.0), 1)


@pytest.fixture(scope="module")
def scenes():
    xyz, rgb = sd.scene()
    out = {s: (vr.create_scene(xyz, rgb, s), oracle.Scene(xyz, rgb, int(s))) for s in (VCS, HASH)}
    yield xyz, rgb, out
    for g, o in out.values():
        g.close()
        o.close()


@pytest.mark.parametrize("light", [x[0] for x in sd.LIGHTS])
@pytest.mark.parametrize("view", list(sd.VIEWS))
def test_view_equals_oracle(scenes, view, light):
    xyz, rgb, both = scenes
    c = sd.case(view, light)
    cam, lit = gpu_camera(c), gpu_lighting(c)
    for store, (g, o) in both.items():
        img = check_frame(xyz, rgb, store, ORIGINAL, W, H, 1, cam=cam, lit=lit, oracle_scene=o, gpu_scene=g)
        assert np.count_nonzero(img) > 100, (view, light, store.name)


@pytest.mark.parametrize("view", list(sd.VIEWS))
def test_generic_walk_agrees(scenes, view):
    """Cluster store, shadows off: the frame the oracle renders is the shading of the records
    that vr_pick (the generic loop) reports for the frame's central tiles -- where the sign
    patterns meet -- and for a stride of the rest; vr_trace of the same rays gives the same bytes."""
    xyz, rgb, both = scenes
    g, o = both[VCS]
    c = sd.case(view, "noshadow")
    cam, lit = gpu_camera(c), gpu_lighting(c)
    want, _ = o.render(int(ORIGINAL), oracle_camera_from(cam), oracle_lighting_from(lit), W, H, 1)
    i = np.arange(W * H)
    x, y = i % W, i // W
    pick = ((abs(x - W // 2) <= 8) & (abs(y - H // 2) <= 8)) | (i % 37 == 0)
    px, py = x[pick].astype(np.uint32), y[pick].astype(np.uint32)
    recs = vr.pick(g, ORIGINAL, cam, INFO, W, H, px, py)
    ps, plit = pyref.Scene(xyz, rgb, int(VCS)), pyref_lighting(c)
    shaded = np.array([pick_ref.shade(ps, r, plit) for r in recs], dtype=np.uint32)
    assert np.array_equal(shaded, want[pick]), diff_report(shaded, want[pick], len(px))
    assert np.count_nonzero(recs["status"] == vr.HitStatus.VOXEL) > 20
    assert np.count_nonzero(recs["status"] == vr.HitStatus.MISS) > 20
    traced = vr.trace(g, ORIGINAL, INFO, vr.camera_rays(cam, W, H, px, py))
    assert pick_ref.same_records(traced, recs).size == 0


@pytest.mark.parametrize("store", [VCS, HASH], ids=lambda s: s.name)
def test_odd_row_range(scenes, store):
    xyz, rgb, both = scenes
    g, o = both[store]
    c = sd.case("plus-x-inside", "oct-pnp")
    check_frame(xyz, rgb, store, ORIGINAL, W, H, 1, cam=gpu_camera(c), lit=gpu_lighting(c), row_begin=29, row_end=58,
                oracle_scene=o, gpu_scene=g)


@pytest.mark.parametrize("store", [VCS, HASH], ids=lambda s: s.name)
def test_tile_deal(scenes, store):
    """The 2-D tile deal over three ranks (16-row bands, 16-column blocks), assembled on the device."""
    xyz, rgb, both = scenes
    g, o = both[store]
    c = sd.case("minus-z", "eq-neg")
    cam, lit = gpu_camera(c), gpu_lighting(c)
    want, _ = o.render(int(ORIGINAL), oracle_camera_from(cam), oracle_lighting_from(lit), W, H, 1)
    R, B, T = 3, 16, 16
    words = vr.tile_buffer_words(W, H, B, T, R)
    parts = torch.full((R, words), -7, dtype=torch.int32, device="cuda")
    for r in range(R):
        vr.render_tiles(g, ORIGINAL, cam, lit, INFO, W, H, B, T, r, R, parts[r])
    frame = torch.empty((H, W), dtype=torch.int32, device="cuda")
    vr.assemble_tiles_device(parts, frame, 4, W, H, B, T, R)
    torch.cuda.synchronize()
    img = frame.cpu().numpy().view(np.uint32).reshape(-1)
    assert np.array_equal(img, want), diff_report(img, want, W)
