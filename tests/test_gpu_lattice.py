"""GPU parity for walks that start on the voxel lattice (tests/lattice_cases.py, whose CPU
preconditions tests/test_lattice_cases.py asserts): views whose every pixel starts on a voxel
face, a cluster plane, a region plane or a face of the frame, held to the oracle as the fuzz
holds its cases (check_frame); vr.pick over every pixel of those views and vr.trace of rays from
lattice points, from one ulp beside them, from scaled and translated forms of both and from the
hit points of first hits, held to the numpy reference record by record, field by field; and the
coherent order at sizes where the sort behind it runs over several workgroups."""
from __future__ import annotations

import numpy as np
import pytest

import oracle
from tests import lattice_cases as lc
from tests import pick_ref
from tests.cover_run import gpu_camera, gpu_lighting
from tests.helpers import oracle_camera_from, oracle_lighting_from
from tests.test_gpu_parity import ALGOS, STORES, check_frame

pytestmark = pytest.mark.gpu

vr = pytest.importorskip("voxelraymarcher_amd")

LONGEST = vr.RayMarchAlgorithm.LONGEST_AXIS
ORDERS = (vr.TraceOrder.GIVEN, vr.TraceOrder.COHERENT)
PAIRS = [(s, a) for s in STORES for a in ALGOS]


def assert_same(got, want, where):
    bad = pick_ref.same_records(got, want)
    assert bad.size == 0, (f"{where}: {bad.size} of {len(got)} records differ; first at {int(bad[0])}: "
                           f"gpu {got[bad[0]]} reference {want[bad[0]]}")


@pytest.fixture(scope="module")
def scenes():
    """The lattice scene on the GPU, one per store (the tests share them: none edits)."""
    out = {s: vr.create_scene(*lc.scene_voxels(), s) for s in STORES}
    yield out
    for s in out.values():
        s.close()


@pytest.mark.parametrize("name", list(lc.VIEWS))
def test_lattice_views(name, scenes):
    """Every view, every store x algorithm, pixels and algorithmic bytes against the oracle: every
    kernel, counted and uncounted launches, relaunches under learned orders; the view with the
    3 x 10^5 iteration crawl also with a deferral list of one entry, which overflows."""
    v = lc.VIEWS[name]
    cam, lit = gpu_camera(v), lc.set_point_light(gpu_lighting(v), v)
    caps = (0, 1) if name == lc.LONG_CRAWL else (0,)
    for store in STORES:
        ref = oracle.Scene(v.xyz, v.rgb, int(store))
        for algo in ALGOS:
            want = ref.render(int(algo), oracle_camera_from(cam), oracle_lighting_from(lit), v.W, v.H, v.scale,
                              v.translation)
            check_frame(v.xyz, v.rgb, store, algo, v.W, v.H, v.scale, cam=cam, lit=lit, translation=v.translation,
                        gpu_scene=scenes[store], want=want, defer_caps=caps)
            if name == lc.UPPER_FACE:
                assert not want[0].any()
            else:
                assert np.count_nonzero(want[0]) >= 200
        ref.close()


@pytest.mark.parametrize("name", list(lc.VIEWS))
def test_lattice_picks(name, scenes):
    """vr.pick over every pixel against tests/pick_ref.py, on the views on which
    tests/test_lattice_cases.py::test_pick_reference_agrees_with_oracle holds that reference to
    the oracle (all but the long crawl); and on every view trace(camera_rays(pixels)) is the pick,
    byte for byte."""
    v = lc.VIEWS[name]
    cam = gpu_camera(v)
    px, py = lc.frame_pixels()
    info = vr.VoxelSceneInfo(v.translation, v.scale)
    rays = vr.camera_rays(cam, v.W, v.H, px, py)
    for store, algo in PAIRS:
        got = vr.pick(scenes[store], algo, cam, info, v.W, v.H, px, py)
        for order in ORDERS:
            again = vr.trace(scenes[store], algo, info, rays, order=order)
            assert again.tobytes() == got.tobytes(), (store, algo, order)
        if name not in lc.TIED:
            continue
        with np.errstate(all="ignore"):
            want, _ = pick_ref.pick_pixels(lc.reference_scene(int(store)), cam, v.W, v.H, px, py, v.scale,
                                           algo == LONGEST, v.translation)
        assert_same(got, want, f"{name} {store.name}/{algo.name}")
        hits = np.count_nonzero(got["status"] == vr.HitStatus.VOXEL)
        assert hits == 0 if name == lc.UPPER_FACE else hits >= 200


@pytest.mark.parametrize("form", list(lc.FORMS))
@pytest.mark.parametrize("family", list(lc.FAMILIES))
def test_lattice_traces(family, form, scenes):
    """Rays from lattice points and from one ulp beside them, at scale 1, at scale 2 (which lands
    on the same origins exactly) and at scale 3 (which makes near-lattice origins of its own):
    the reference's records under both orders."""
    scale, tr = lc.FORMS[form]
    rays = lc.family_rays(family, form)
    info = vr.VoxelSceneInfo(tr, scale)
    for store, algo in PAIRS:
        with np.errstate(all="ignore"):
            want, _ = lc.reference(family, form, int(store), algo == LONGEST)
        for order in ORDERS:
            got = vr.trace(scenes[store], algo, info, rays, order=order)
            assert_same(got, want, f"{family} {form} {store.name}/{algo.name} {order.name}")
        assert not (got["status"] == vr.HitStatus.OUTSIDE).any()


@pytest.mark.parametrize("form", lc.BOUNCE_FORMS)
def test_bounce_traces(form, scenes):
    """Rays from a pick's `point`: the GPU's first hits of the lattice rays are the reference's,
    so the bounce rays made of either are the same rays; their records are the reference's."""
    scale, tr = lc.FORMS[form]
    first_rays = lc.family_rays("lattice", form)
    info = vr.VoxelSceneInfo(tr, scale)
    for store, algo in PAIRS:
        longest = algo == LONGEST
        with np.errstate(all="ignore"):
            first_want, _ = lc.reference("lattice", form, int(store), longest)
            rays, src, want, _ = lc.bounce_reference(form, int(store), longest)
        first = vr.trace(scenes[store], algo, info, first_rays)
        assert_same(first, first_want, f"first hits {form} {store.name}/{algo.name}")
        own, own_src = lc.bounce_rays(first, first_rays, scale, tr)
        assert own.tobytes() == rays.tobytes() and np.array_equal(own_src, src)
        for order in ORDERS:
            got = vr.trace(scenes[store], algo, info, own, order=order)
            assert_same(got, want, f"bounce {form} {store.name}/{algo.name} {order.name}")
        assert np.count_nonzero(got["status"] == vr.HitStatus.VOXEL) >= len(own) // 5


SINGLE_WORKGROUP_SORT, MERGE_SORT_LIMIT = 1024, 1024 * 1024
SORT_SIZES = (4099, 300_001, MERGE_SORT_LIMIT + 1001)


@pytest.mark.parametrize("n", SORT_SIZES)
def test_coherent_order_at_scale(n, scenes):
    """The coherent order where the sort behind it leaves the single workgroup.  The rays are the
    lattice rays repeated and shuffled (so every key repeats): COHERENT returns GIVEN's bytes, and
    record i is the reference's record of the ray it repeats.

    n = 4 099 and 300 001 take rocprim's merge-sort path (a block sort and merge passes over several
    workgroups), n = 1024 * 1024 + 1001 = 1 049 577 its Onesweep path; none is a multiple of 256.
    rocprim::radix_sort_pairs with the default config, 64-bit keys and 32-bit values, chooses in
    radix_sort_impl (rocprim/device/device_radix_sort.hpp):
      "if(size <= static_cast<decltype(size)>(single_sort_items_per_block))": one workgroup, where
        single_sort_items_per_block = block_size * items_per_thread of "kernel_config<rocprim::min(
        256u, ...block_size), rocprim::min(4u, ...items_per_thread)>" over
        radix_sort_block_sort_config_base<Key, Value> (device/detail/device_config_helper.hpp):
        item_scale = max(sizeof(Key), sizeof(Value)) = 8 gives merge_sort_block_size(8) * 2 = 256
        threads and min(4, merge_sort_items_per_thread(8) = 4) = 4 items each: 1024 items;
      "else if(static_cast<size_t>(size) <= merge_sort_limit && (sizeof(key_type) > 2 || size <
        100000) && !using_spirv)": merge sort, with radix_sort_config's "size_t MergeSortLimit =
        1024 * 1024" (device/device_radix_sort_config.hpp);
      else Onesweep."""
    assert n > SINGLE_WORKGROUP_SORT and (n <= MERGE_SORT_LIMIT or n == SORT_SIZES[-1]) and n % 256 != 0
    assert min(SORT_SIZES) <= MERGE_SORT_LIMIT < max(SORT_SIZES)
    store, algo = vr.StorageType.VOXEL_CLUSTER_STORE, LONGEST
    base = lc.family_rays("lattice", "scale1")
    with np.errstate(all="ignore"):
        want, _ = lc.reference("lattice", "scale1", int(store), True)
    idx = np.random.default_rng(n).permutation(np.arange(n) % len(base))
    rays = base[idx]
    info = vr.VoxelSceneInfo(lc.ZERO, 1)
    given = vr.trace(scenes[store], algo, info, rays, order=vr.TraceOrder.GIVEN)
    assert_same(given, want[idx], f"n = {n}, GIVEN")
    coherent = vr.trace(scenes[store], algo, info, rays, order=vr.TraceOrder.COHERENT)
    assert coherent.tobytes() == given.tobytes()
