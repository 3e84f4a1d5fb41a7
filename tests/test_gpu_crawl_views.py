"""Directed crawl views against the oracle (tests/crawl_views.py): 48x32 frames in which
dozens of pixels are cluster-skip crawls of 65 536 to ~10^6 iterations -- on each axis's
cluster planes, in primary and in shadow walks, at scale 2 with a translation, under a
point light -- so the tile pass defers them and the crawl pass fast-forwards them
(vr_crawl.h).  The CPU test holds the views to that description with the oracle alone;
the GPU tests compare pixels and algorithmic bytes bit-exactly, through both deferral
forms and with a deferral list that overflows."""
from __future__ import annotations

import numpy as np
import pytest

import oracle
from tests.crawl_views import ASPECT, H, LONG_WALK, MIN_LONG_PIXELS, SCENES, UP, VIEWS, W

ALGOS = [oracle.ALGO_ORIGINAL, oracle.ALGO_LONGESTAXIS]
ALGO_IDS = {oracle.ALGO_ORIGINAL: "ORIGINAL", oracle.ALGO_LONGESTAXIS: "LONGEST_AXIS"}

_voxels: dict = {}


def voxels(name):
    if name not in _voxels:
        _voxels[name] = SCENES[name]()
    return _voxels[name]


def oracle_view(view):
    """The view's camera and lighting block built by the oracle's own host code."""
    cam = oracle.camera(view.world(view.eye), view.world(view.look_at), UP, view.fov, ASPECT)
    lit = oracle.lighting(True, view.point, view.light_pos)
    if view.light_dir is not None:        # makeUnitVector in float32 (Vector3.cuh:162)
        d = np.array(view.light_dir, dtype=np.float32)
        n = np.sqrt(np.float32(np.float32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
        for i in range(3):
            lit.light_dir[i] = float(np.float32(d[i] / n))
    return cam, lit


@pytest.mark.parametrize("algo", ALGOS, ids=ALGO_IDS.get)
@pytest.mark.parametrize("view", VIEWS, ids=lambda v: v.name)
def test_views_crawl_in_the_oracle(view, algo):
    """Each primary view has >= 20 pixels whose primary walk runs >= 65 536 iterations, each
    shadow view >= 5 pixels whose shadow walk does (oracle.Scene.pixel_stats).  A view that
    stops crawling is replaced by one that does, not excused."""
    ref = oracle.Scene(*voxels(view.scene), oracle.STORE_VCS)
    cam, lit = oracle_view(view)
    iters = ref.pixel_stats(algo, cam, lit, W, H, view.scale, view.translation)[..., 6]
    n_long = int(np.count_nonzero(iters[..., 1 if view.shadow else 0] >= LONG_WALK))
    print(f"{view.name} {ALGO_IDS[algo]}: {n_long} long {'shadow' if view.shadow else 'primary'} walks, "
          f"longest {int(iters.max())} iterations")
    assert n_long >= MIN_LONG_PIXELS[view.shadow]
    ref.close()


@pytest.fixture(scope="module")
def scenes():
    """Per scene: the voxels, the GPU scene and the oracle scene, built once."""
    vr = pytest.importorskip("voxelraymarcher_amd")
    made = {}

    def get(name):
        if name not in made:
            xyz, rgb = voxels(name)
            made[name] = (xyz, rgb, vr.create_scene(xyz, rgb, vr.StorageType.VOXEL_CLUSTER_STORE),
                          oracle.Scene(xyz, rgb, oracle.STORE_VCS))
        return made[name]
    yield get
    for _, _, g, o in made.values():
        g.close()
        o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ALGOS, ids=ALGO_IDS.get)
@pytest.mark.parametrize("view", VIEWS, ids=lambda v: v.name)
def test_crawl_view_matches_oracle(scenes, view, algo):
    """Pixels and algorithmic bytes of the crawling frame: kernels TILE (deferred walks
    resume at the crawl) and TILE_REWALK (they walk from their start), deferral list
    unbounded and of 4 records (it overflows: the crawl pass scans the frame).  Then three
    more plain renders of the same view -- the launches that use what the first ones
    learned (crawl-pass skip, tile and lane orders) -- still give the oracle's frame."""
    import voxelraymarcher_amd as vr
    from tests.helpers import diff_report, gpu_render
    from tests.test_gpu_parity import check_frame

    xyz, rgb, gpu, ref = scenes(view.scene)
    valgo = vr.RayMarchAlgorithm(algo)
    cam = vr.Camera(view.world(view.eye), view.world(view.look_at), UP, view.fov, ASPECT)
    lit = vr.setup_constant_values(use_point_light=view.point, light_position=view.light_pos,
                                   light_direction=view.light_dir)
    want = check_frame(xyz, rgb, vr.StorageType.VOXEL_CLUSTER_STORE, valgo, W, H, view.scale, cam=cam, lit=lit,
                       translation=view.translation, count=True, oracle_scene=ref, gpu_scene=gpu,
                       kernels=[vr.Kernel.TILE, vr.Kernel.TILE_REWALK], defer_caps=(0, 4))
    info = vr.VoxelSceneInfo(view.translation, view.scale)
    for i in range(3):
        got, _ = gpu_render(gpu, valgo, cam, lit, info, W, H)
        assert np.array_equal(got, want), f"render {i + 2} of the view: " + diff_report(got, want, W)
