"""Host-side interface of the renderer, mirroring the reference's host names.

  StorageType            geometry/VoxelFunctions.cuh:37
  Camera                 renderer/camera/Camera.cuh:11-29
  VoxelSceneInfo         renderer/VoxelSceneInfo.cuh:5-15
  VoxelSceneCPU          geometry/VoxelSceneCPU.cuh:13-131 (insertVoxel, generateVoxelScene)
  read_voxel_file        geometry/VoxelFile.cuh:9-35
  setup_constant_values  main/Main.cu:26-42
  run_raymarching_kernel main/Main.cu:105-163

All compute goes through libvr.so (HIP, gfx950).  Device buffers are torch
tensors (plumbing only); frames are uint32 tensors of packed 0x00RRGGBB words.
"""
from __future__ import annotations

import ctypes
import enum
from ctypes import c_int32, c_size_t, c_uint32, c_void_p
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _capi
from ._capi import check, f3, lib


class StorageType(enum.IntEnum):
    VOXEL_CLUSTER_STORE = _capi.VR_STORE_VCS
    HASH_TABLE = _capi.VR_STORE_HASHTABLE


class RayMarchAlgorithm(enum.IntEnum):
    LONGEST_AXIS = _capi.VR_ALGO_LONGESTAXIS
    ORIGINAL = _capi.VR_ALGO_ORIGINAL


def parse_storage(name: str) -> StorageType:
    """processStorageTypeCmdArg (Main.cu:45-55): 'hashtable' else VCS."""
    return StorageType.HASH_TABLE if name == "hashtable" else StorageType.VOXEL_CLUSTER_STORE


def parse_algorithm(name: str) -> RayMarchAlgorithm:
    """processAlgorithmCmdArg (Main.cu:58-68): 'original' else longest axis."""
    return RayMarchAlgorithm.ORIGINAL if name == "original" else RayMarchAlgorithm.LONGEST_AXIS


class Camera:
    """Camera(o, lookAt, globalUp, fieldOfView, aspectRatio) (Camera.cuh:11-23), built on the host."""

    def __init__(self, origin, look_at, global_up, field_of_view: float, aspect_ratio: float):
        self.raw = _capi.VrCamera()
        check(lib().vr_camera_make(f3(origin), f3(look_at), f3(global_up), float(field_of_view),
                                   float(aspect_ratio), ctypes.byref(self.raw)), "Camera")

    @classmethod
    def reference(cls, width: int, height: int) -> "Camera":
        """The hard-coded camera of Main.cu:197-199."""
        aspect = float(np.float32(width) / np.float32(height))
        return cls((6.0, 2.0, 6.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 60.0, aspect)

    def as_floats(self) -> np.ndarray:
        r = self.raw
        return np.array([list(r.origin), list(r.lower_left), list(r.horizontal), list(r.vertical),
                         list(r.forward)], dtype=np.float32)


def setup_constant_values(use_shadows: bool = True, use_point_light: bool = False,
                          light_position=(10.0, 10.0, -10.0), light_direction=None,
                          light_color=(1.0, 1.0, 1.0)) -> _capi.VrLighting:
    """setupConstantValues (Main.cu:26-42) -> the lighting block. The defaults are
    the reference's; `light_direction` (un-normalised, default (1,1,1)) goes through
    makeUnitVector exactly as Main.cu:28 does it."""
    lit = _capi.VrLighting()
    check(lib().vr_lighting_default(ctypes.byref(lit)), "setupConstantValues")
    if light_direction is not None:
        d = (ctypes.c_float * 3)(*[float(c) for c in light_direction])
        check(lib().vr_lighting_set_direction(ctypes.byref(lit), d), "light direction")
    lit.use_shadows = int(bool(use_shadows))
    lit.use_point_light = int(bool(use_point_light))
    for i in range(3):
        lit.light_pos[i] = float(light_position[i])
        lit.light_color[i] = float(light_color[i])
    return lit


@dataclass
class VoxelSceneInfo:
    """VoxelSceneInfo(location, scale) (VoxelSceneInfo.cuh:5-15)."""
    translation: tuple = (0.0, 0.0, 0.0)
    scale: int = 1


VOXEL_REMOVE = 0xFFFFFFFF   # VR_VOXEL_REMOVE: as an edit's colour, delete the voxel
VOXEL_ABSENT = 0xFFFFFFFF   # VR_VOXEL_ABSENT: a lookup's answer for a voxel that is not stored


def _voxel_batch(xyz, rgb):
    """The (xyz, rgb) batch of edit() and paint() as (int32 [n,3], 32-bit [n], on_device):
    contiguous CUDA tensors when xyz is one, numpy arrays otherwise."""
    if hasattr(xyz, "is_cuda") and xyz.is_cuda:
        xyz = xyz.to(torch.int32).contiguous().reshape(-1, 3)
        rgb = rgb.contiguous().reshape(-1)
        if rgb.dtype not in (torch.int32, torch.uint32):
            # (VOXEL_REMOVE does not fit int32: wrap int64 colours to 32 bits)
            rgb = ((((rgb.to(torch.int64) & 0xFFFFFFFF) ^ 0x80000000) - 0x80000000).to(torch.int32)).contiguous()
        dev = 1
    else:
        xyz = np.ascontiguousarray(xyz, dtype=np.int32).reshape(-1, 3)
        rgb = np.ascontiguousarray(rgb, dtype=np.uint32).reshape(-1)
        dev = 0
    if xyz.shape[0] != rgb.shape[0]:
        raise ValueError("xyz and rgb lengths differ")
    return xyz, rgb, dev


class DeviceScene:
    """One scene resident in HBM (owns the vr_scene handle); changed only by edit()."""

    def __init__(self, handle: c_void_p):
        self._h = handle

    @property
    def handle(self) -> c_void_p:
        if not self._h:
            raise ValueError("scene destroyed")
        return self._h

    def info(self) -> dict:
        i = _capi.VrSceneInfo()
        check(lib().vr_scene_get_info(self.handle, ctypes.byref(i)), "vr_scene_get_info")
        return {"diameter": i.diameter, "min_coord": i.min_coord, "region_count": i.region_count,
                "store": StorageType(i.store), "voxel_count": i.voxel_count, "device_bytes": i.device_bytes,
                "device": i.device}

    def digest(self) -> tuple:
        """FNV-1a of (region table, VCS masks, VCS colours, cuckoo meta, cuckoo slots)."""
        d = (ctypes.c_uint64 * 5)()
        check(lib().vr_scene_digest(self.handle, d), "vr_scene_digest")
        return tuple(int(x) for x in d)

    def edit(self, xyz, rgb, stream=None) -> None:
        """vr_scene_edit: apply the edits in order, in place.  Edit i sets voxel xyz[i] to
        colour rgb[i] (< 2^24) or, with VOXEL_REMOVE, deletes it; later edits of a coordinate
        win.  xyz/rgb: numpy arrays, or torch tensors on the scene's device.  All or nothing
        (VrError leaves the scene as it was); runs on `stream` (default: the current stream)
        and returns when the scene is ready.  With several GPUs every rank holds its own
        scene: the same batch applied on every rank gives identical images."""
        sp = _stream_ptr(stream)
        xyz, rgb, dev = _voxel_batch(xyz, rgb)
        check(lib().vr_scene_edit(self.handle, _ptr(xyz), _ptr(rgb), rgb.shape[0], dev, sp), "vr_scene_edit")

    def lookup(self, xyz, stream=None):
        """vr_scene_lookup: the stored colour of each world voxel xyz[i], or VOXEL_ABSENT -- for
        any int32 coordinates, inside the scene's frame or not.  A numpy array (or list) gives
        numpy uint32[n]; a CUDA tensor on the scene's device gives an int32 tensor there with
        the same words (VOXEL_ABSENT reads as -1).  Runs on `stream` (default: the current
        stream) and returns when the colours are written; no render launch."""
        dev = int(hasattr(xyz, "is_cuda") and xyz.is_cuda)
        if dev:
            xyz = xyz.to(torch.int32).contiguous().reshape(-1, 3)
            rgb = torch.empty(xyz.shape[0], dtype=torch.int32, device=xyz.device)
        else:
            xyz = np.ascontiguousarray(xyz, dtype=np.int32).reshape(-1, 3)
            rgb = np.zeros(xyz.shape[0], dtype=np.uint32)
        if xyz.shape[0]:
            check(lib().vr_scene_lookup(self.handle, _ptr(xyz), xyz.shape[0], dev, _ptr(rgb), dev, _stream_ptr(stream)),
                  "vr_scene_lookup")
        return rgb

    def paint(self, xyz, rgb, stream=None) -> int:
        """vr_scene_paint: recolour stored voxels in place.  Edit i sets voxel xyz[i] to colour
        rgb[i] (< 2^24) if it is stored; later edits of a coordinate win.  Returns the number of
        edits whose voxel is not stored (they do nothing: a paint never inserts or removes).
        xyz/rgb as for edit().  A colour >= 2^24 raises VrError and leaves the scene as it was.
        O(n), no rebuild, and -- unlike edit() -- the scene's views keep what the renderer has
        learned about them.  Runs on `stream` (default: the current stream) and returns when the
        colours are written."""
        sp = _stream_ptr(stream)
        xyz, rgb, dev = _voxel_batch(xyz, rgb)
        absent = c_size_t(0)
        check(lib().vr_scene_paint(self.handle, _ptr(xyz), _ptr(rgb), rgb.shape[0], dev, sp, ctypes.byref(absent)),
              "vr_scene_paint")
        return int(absent.value)

    def voxels(self, device: bool = False, stream=None):
        """vr_scene_voxels: the scene's voxels, (xyz int32[n,3], rgb uint32[n]) as numpy arrays,
        or (device=True) as torch tensors on the scene's device (rgb as int32 words).  Ordered
        by region index, then by the store's key order."""
        n = c_size_t()
        check(lib().vr_scene_voxels(self.handle, None, None, 0, 0, None, ctypes.byref(n)), "vr_scene_voxels")
        sp = _stream_ptr(stream)
        if device:
            dev = torch.device("cuda", self.info()["device"])
            xyz = torch.empty((n.value, 3), dtype=torch.int32, device=dev)
            rgb = torch.empty(n.value, dtype=torch.int32, device=dev)
            if n.value:
                check(lib().vr_scene_voxels(self.handle, c_void_p(xyz.data_ptr()), c_void_p(rgb.data_ptr()), n.value, 1,
                                            sp, ctypes.byref(n)), "vr_scene_voxels")
            return xyz, rgb
        xyz = np.zeros((max(n.value, 1), 3), dtype=np.int32)
        rgb = np.zeros(max(n.value, 1), dtype=np.uint32)
        check(lib().vr_scene_voxels(self.handle, xyz.ctypes.data_as(c_void_p), rgb.ctypes.data_as(c_void_p), n.value, 0,
                                    sp, ctypes.byref(n)), "vr_scene_voxels")
        return xyz[: n.value].copy(), rgb[: n.value].copy()

    def pick(self, algorithm, camera, info, width: int, height: int, px, py, stream=None):
        """vr_pick with this scene: see pick()."""
        return pick(self, algorithm, camera, info, width, height, px, py, stream=stream)

    def trace(self, algorithm, info, rays, order=None, stream=None):
        """vr_trace with this scene: see trace()."""
        return trace(self, algorithm, info, rays, order=TraceOrder.AUTO if order is None else order, stream=stream)

    def shade(self, algorithm, info, lighting, rays, order=None, hits: bool = False, stream=None):
        """vr_shade with this scene: see shade()."""
        return shade(self, algorithm, info, lighting, rays, order=TraceOrder.AUTO if order is None else order,
                     hits=hits, stream=stream)

    def shade_lights(self, algorithm, info, lights, rays, ambient=None, order=None, hits: bool = False, stream=None,
                     ao=None, ao_apply=None, return_ao: bool = False, reflect=None, bounces: int = 1, mirror=None,
                     atmosphere=None):
        """vr_shade_lights (or, with ao=, vr_shade_lights_ao; with reflect=, vr_shade_lights_reflect; with
        atmosphere=, vr_shade_lights_atmosphere) with this scene: see shade_lights()."""
        return shade_lights(self, algorithm, info, lights, rays, ambient=ambient, order=order, hits=hits, stream=stream,
                            ao=ao, ao_apply=ao_apply, return_ao=return_ao, reflect=reflect, bounces=bounces, mirror=mirror,
                            atmosphere=atmosphere)

    def occlusion(self, hits, stream=None):
        """vr_occlusion with this scene: see occlusion()."""
        return occlusion(self, hits, stream=stream)

    def close(self) -> None:
        if self._h:
            lib().vr_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Build(enum.IntEnum):
    """vr_build: where the scene image is built (both give identical images)."""
    AUTO = 0
    DEVICE = 1
    HOST = 2


def _build_stream(stream) -> c_void_p:
    return c_void_p(None) if stream is None else c_void_p(stream.cuda_stream)


def create_scene(xyz, rgb, store: StorageType, device: int = 0, build: Build = Build.AUTO, stream=None) -> DeviceScene:
    """generateVoxelScene(storageType) over the voxels (VoxelSceneCPU.cuh:49-93).
    xyz/rgb: numpy arrays, or torch tensors already on the GPU (int32 [n,3] / [n])."""
    h = c_void_p()
    if hasattr(xyz, "is_cuda") and xyz.is_cuda:
        import torch
        xyz = xyz.to(torch.int32).contiguous().reshape(-1, 3)
        rgb = rgb.to(torch.int32).contiguous().reshape(-1)
        if xyz.shape[0] != rgb.shape[0]:
            raise ValueError("xyz and rgb lengths differ")
        check(lib().vr_scene_create_ex(int(device), int(store), c_void_p(xyz.data_ptr()), c_void_p(rgb.data_ptr()),
                                       rgb.shape[0], 1, int(build), _build_stream(stream), ctypes.byref(h)),
              "generateVoxelScene")
        return DeviceScene(h)
    xyz = np.ascontiguousarray(xyz, dtype=np.int32).reshape(-1, 3)
    rgb = np.ascontiguousarray(rgb, dtype=np.uint32).reshape(-1)
    if xyz.shape[0] != rgb.shape[0]:
        raise ValueError("xyz and rgb lengths differ")
    check(lib().vr_scene_create_ex(int(device), int(store), xyz.ctypes.data_as(ctypes.c_void_p),
                                   rgb.ctypes.data_as(ctypes.c_void_p), rgb.shape[0], 0, int(build),
                                   _build_stream(stream), ctypes.byref(h)),
          "generateVoxelScene")
    return DeviceScene(h)


class VoxelSceneCPU:
    """Host-side voxel accumulator (VoxelSceneCPU.cuh:13-46)."""

    def __init__(self):
        self._xyz: list = []
        self._rgb: list = []

    def insert_voxel(self, x: int, y: int, z: int, color: int) -> None:
        self._xyz.append((int(x), int(y), int(z)))
        self._rgb.append(int(color) & 0xFFFFFFFF)

    insertVoxel = insert_voxel

    def extend(self, xyz: np.ndarray, rgb: np.ndarray) -> None:
        self._xyz.extend(map(tuple, np.asarray(xyz, dtype=np.int64).reshape(-1, 3).tolist()))
        self._rgb.extend(np.asarray(rgb, dtype=np.uint64).reshape(-1).tolist())

    def arrays(self):
        return (np.array(self._xyz, dtype=np.int32).reshape(-1, 3), np.array(self._rgb, dtype=np.uint32))

    def generate_voxel_scene(self, storage_type: StorageType, device: int = 0) -> DeviceScene:
        xyz, rgb = self.arrays()
        return create_scene(xyz, rgb, storage_type, device)

    generateVoxelScene = generate_voxel_scene


def _read_scene_file(fn: str, path: str):
    n = c_size_t()
    check(getattr(lib(), fn)(path.encode(), None, None, 0, ctypes.byref(n)), fn)
    xyz = np.zeros((max(n.value, 1), 3), dtype=np.int32)
    rgb = np.zeros(max(n.value, 1), dtype=np.uint32)
    check(getattr(lib(), fn)(path.encode(), xyz.ctypes.data_as(ctypes.POINTER(c_int32)),
                             rgb.ctypes.data_as(ctypes.POINTER(c_uint32)), n.value, ctypes.byref(n)), fn)
    return xyz[: n.value].copy(), rgb[: n.value].copy()


def read_voxel_file(path: str):
    """VoxelFile::readVoxelFile (VoxelFile.cuh:9-35) -> (xyz int32[n,3], rgb uint32[n]).
    Reads the .vox CSV (parsed in parallel, same rules) or, detected by its magic,
    the .vxb binary sidecar."""
    return _read_scene_file("vr_scene_file_read", path)


def write_voxel_file(path: str, xyz: np.ndarray, rgb: np.ndarray) -> None:
    xyz = np.ascontiguousarray(xyz, dtype=np.int32).reshape(-1, 3)
    rgb = np.ascontiguousarray(rgb, dtype=np.uint32).reshape(-1)
    check(lib().vr_vox_write(path.encode(), xyz.ctypes.data_as(ctypes.POINTER(c_int32)),
                             rgb.ctypes.data_as(ctypes.POINTER(c_uint32)), rgb.shape[0]), "write_voxel_file")


def write_binary_scene(path: str, xyz: np.ndarray, rgb: np.ndarray) -> None:
    """The .vxb binary sidecar (vr_vxb_write): the same voxels, loaded without parsing."""
    xyz = np.ascontiguousarray(xyz, dtype=np.int32).reshape(-1, 3)
    rgb = np.ascontiguousarray(rgb, dtype=np.uint32).reshape(-1)
    check(lib().vr_vxb_write(path.encode(), xyz.ctypes.data_as(ctypes.POINTER(c_int32)),
                             rgb.ctypes.data_as(ctypes.POINTER(c_uint32)), rgb.shape[0]), "write_binary_scene")


def synth_scene(n: int, p_region: float, p_cluster: float, p_voxel: float, seed: int):
    """Synthetic counter-hash grid -> (xyz int32[n,3], rgb uint32[n])."""
    p = _capi.VrSynthParams(int(n), float(p_region), float(p_cluster), float(p_voxel), int(seed))
    cnt = c_size_t()
    check(lib().vr_synth_generate(ctypes.byref(p), None, None, 0, ctypes.byref(cnt)), "vr_synth_generate")
    xyz = np.zeros((max(cnt.value, 1), 3), dtype=np.int32)
    rgb = np.zeros(max(cnt.value, 1), dtype=np.uint32)
    check(lib().vr_synth_generate(ctypes.byref(p), xyz.ctypes.data_as(ctypes.POINTER(c_int32)),
                                  rgb.ctypes.data_as(ctypes.POINTER(c_uint32)), cnt.value, ctypes.byref(cnt)),
          "vr_synth_generate")
    return xyz[: cnt.value].copy(), rgb[: cnt.value].copy()


def _stream_ptr(stream) -> c_void_p:
    if stream is None:
        stream = torch.cuda.current_stream()
    return c_void_p(stream.cuda_stream)


def _require_u32(out: torch.Tensor, words: int) -> None:
    if not out.is_cuda or out.dtype != torch.int32 and out.dtype != torch.uint32:
        raise TypeError("out must be a CUDA int32/uint32 tensor")
    if not out.is_contiguous() or out.numel() < words:
        raise ValueError(f"out must be contiguous with >= {words} elements")


class Kernel(enum.IntEnum):
    """vr_kernel: which HIP implementation renders (identical pixels)."""
    AUTO = _capi.VR_KERNEL_AUTO
    TILE = _capi.VR_KERNEL_TILE
    TILE_REWALK = _capi.VR_KERNEL_TILE_REWALK


class Schedule(enum.IntEnum):
    """vr_schedule: the tile pass's work order (identical pixels).  AUTO: heaviest tile
    groups first when the device's previous launch was on the same stream or has finished
    (a lone frame's latency), grid order while another stream's launch runs (frames in flight)."""
    AUTO = _capi.VR_SCHEDULE_AUTO
    GRID = _capi.VR_SCHEDULE_GRID
    HEAVIEST_FIRST = _capi.VR_SCHEDULE_HEAVIEST_FIRST


class Occupancy(enum.IntEnum):
    """vr_occupancy: the tile pass's occupancy variant (identical pixels).  AUTO: the in-flight
    variant while another stream's launch runs -- where one is built (vr_march.hip
    VR_ORIG_WAVES_HI / VR_LONG_WAVES_HI; round 6 measured every walk fastest in flight with its
    lone kernel, so by default IN_FLIGHT launches that kernel)."""
    AUTO = _capi.VR_OCCUPANCY_AUTO
    LONE = _capi.VR_OCCUPANCY_LONE
    IN_FLIGHT = _capi.VR_OCCUPANCY_IN_FLIGHT


def render_ex(scene: DeviceScene, algorithm: RayMarchAlgorithm, camera: Camera, lighting: _capi.VrLighting,
              info: VoxelSceneInfo, width: int, height: int, out: torch.Tensor, row_begin: int = 0,
              row_end: int | None = None, band_rows: int = 0, rank: int = 0, nranks: int = 1,
              counter: torch.Tensor | None = None, kernel: Kernel = Kernel.AUTO, stream=None,
              defer_cap: int = 0, schedule: Schedule = Schedule.AUTO,
              stats: torch.Tensor | None = None, occupancy: Occupancy = Occupancy.AUTO,
              tile_cols: int = 0, deal_stride: int = 0) -> torch.Tensor:
    """vr_render_ex: rows [row_begin,row_end), bands of band_rows (0 = one band) dealt to nranks ranks.
    defer_cap: capacity of the crawl pass's deferral list (0 = default; small values force its overflow path).
    schedule: the tile pass's work order (Schedule); occupancy: its occupancy variant (Occupancy).
    stats (with counter): CUDA int64[2], caller-zeroed: [0] crawl iterations fast-forwarded in closed form,
    [1] the existence-read bytes credited for them (part of counter's count, never loaded).
    tile_cols > 0: the 2-D tile deal (block j of band b -> rank (j + deal_stride * b) % nranks;
    tile_buffer_words per rank)."""
    row_end = height if row_end is None else row_end
    rows = row_end - row_begin
    if tile_cols:
        words = tile_buffer_words(width, rows, band_rows or max(1, rows), tile_cols, nranks)
    else:
        words = band_buffer_words(width, rows, band_rows or max(1, rows), nranks)
    _require_u32(out, words)
    for name, t in (("counter", counter), ("stats", stats)):
        if t is not None and (not t.is_cuda or t.dtype != torch.int64):
            raise TypeError(f"{name} must be a CUDA int64 tensor")
    if stats is not None and (counter is None or stats.numel() < 2 or not stats.is_contiguous()):
        raise ValueError("stats needs a counter and 2 contiguous int64 elements")
    opts = _capi.VrRenderOpts()
    check(lib().vr_render_opts_init(ctypes.byref(opts)), "vr_render_opts_init")
    opts.kernel, opts.row_begin, opts.row_end = int(kernel), int(row_begin), int(row_end)
    opts.band_rows, opts.rank, opts.nranks = int(band_rows), int(rank), int(nranks)
    opts.bytes_dev = c_void_p(counter.data_ptr()) if counter is not None else None
    opts.defer_cap, opts.schedule = int(defer_cap), int(schedule)
    opts.stats_dev = c_void_p(stats.data_ptr()) if stats is not None else None
    opts.occupancy, opts.tile_cols, opts.deal_stride = int(occupancy), int(tile_cols), int(deal_stride)
    check(lib().vr_render_ex(scene.handle, int(algorithm), ctypes.byref(camera.raw), ctypes.byref(lighting),
                             f3(info.translation), int(info.scale), int(width), int(height), ctypes.byref(opts),
                             c_void_p(out.data_ptr()), _stream_ptr(stream)), "vr_render_ex")
    return out


class PreparedRender:
    """One view's launch with its arguments made once (render_ex's options, without counter
    or stats): calling it enqueues vr_render_ex into `out` on `stream` (a torch stream, or
    None for the current one).  For a frame loop's per-frame host path: render_ex rebuilds
    the options and re-checks the buffer on every call (~20 us of Python per frame, which a
    20-frame timed loop pays up front while the GPU waits for its first frame;
    profiles/r06/driver_probe2.py).  The camera and lighting structs are passed by reference,
    so changing `camera.raw` in place re-aims the next call; out's size is checked once per
    buffer.  `vr_stream_arg`: BandGather hands its slot stream over instead of entering a
    torch stream context."""
    vr_stream_arg = True

    def __init__(self, scene: DeviceScene, algorithm: RayMarchAlgorithm, camera: Camera,
                 lighting: _capi.VrLighting, info: VoxelSceneInfo, width: int, height: int, row_begin: int = 0,
                 row_end: int | None = None, band_rows: int = 0, rank: int = 0, nranks: int = 1,
                 kernel: Kernel = Kernel.AUTO, schedule: Schedule = Schedule.AUTO,
                 occupancy: Occupancy = Occupancy.AUTO, tile_cols: int = 0, deal_stride: int = 0):
        row_end = height if row_end is None else row_end
        rows = row_end - row_begin
        if tile_cols:
            self.words = tile_buffer_words(width, rows, band_rows or max(1, rows), tile_cols, nranks)
        else:
            self.words = band_buffer_words(width, rows, band_rows or max(1, rows), nranks)
        opts = _capi.VrRenderOpts()
        check(lib().vr_render_opts_init(ctypes.byref(opts)), "vr_render_opts_init")
        opts.kernel, opts.row_begin, opts.row_end = int(kernel), int(row_begin), int(row_end)
        opts.band_rows, opts.rank, opts.nranks = int(band_rows), int(rank), int(nranks)
        opts.schedule, opts.occupancy = int(schedule), int(occupancy)
        opts.tile_cols, opts.deal_stride = int(tile_cols), int(deal_stride)
        self._keep = (scene, camera, lighting, opts, f3(info.translation))   # (alive while prepared)
        self._fn = lib().vr_render_ex
        self._args = (scene.handle, int(algorithm), ctypes.byref(camera.raw), ctypes.byref(lighting),
                      self._keep[4], int(info.scale), int(width), int(height), ctypes.byref(opts))
        self._checked = set()

    def __call__(self, out: torch.Tensor, stream=None) -> torch.Tensor:
        key = (out.data_ptr(), out.numel(), out.dtype, out.is_contiguous())
        if key not in self._checked:
            _require_u32(out, self.words)
            if len(self._checked) >= 64:          # (a loop over many buffers: keep the set small)
                self._checked.clear()
            self._checked.add(key)
        sh = (stream if stream is not None else torch.cuda.current_stream()).cuda_stream
        rc = self._fn(*self._args, c_void_p(key[0]), c_void_p(sh))
        if rc:
            check(rc, "vr_render_ex")
        return out


def run_raymarching_kernel(scene: DeviceScene, algorithm: RayMarchAlgorithm, camera: Camera,
                           lighting: _capi.VrLighting, info: VoxelSceneInfo, width: int, height: int,
                           out: torch.Tensor | None = None, row_begin: int = 0, row_end: int | None = None,
                           stream=None, kernel: Kernel = Kernel.AUTO) -> torch.Tensor:
    """Launch the ray march for rows [row_begin,row_end) (Main.cu:105-163); asynchronous."""
    row_end = height if row_end is None else row_end
    words = (row_end - row_begin) * width
    if out is None:
        out = torch.empty(words, dtype=torch.int32, device=f"cuda:{scene.info()['device']}")
    if kernel == Kernel.AUTO:
        _require_u32(out, words)
        check(lib().vr_render(scene.handle, int(algorithm), ctypes.byref(camera.raw), ctypes.byref(lighting),
                              f3(info.translation), int(info.scale), int(width), int(height), int(row_begin),
                              int(row_end), c_void_p(out.data_ptr()), _stream_ptr(stream)), "vr_render")
        return out
    return render_ex(scene, algorithm, camera, lighting, info, width, height, out, row_begin, row_end,
                     kernel=kernel, stream=stream)


def render_count(scene: DeviceScene, algorithm: RayMarchAlgorithm, camera: Camera, lighting: _capi.VrLighting,
                 info: VoxelSceneInfo, width: int, height: int, out: torch.Tensor, counter: torch.Tensor,
                 row_begin: int = 0, row_end: int | None = None, stream=None,
                 kernel: Kernel = Kernel.AUTO) -> None:
    """Instrumented render: adds the SURVEY 8(d) algorithmic bytes into counter (int64 cuda scalar)."""
    render_ex(scene, algorithm, camera, lighting, info, width, height, out, row_begin, row_end,
              counter=counter, kernel=kernel, stream=stream)


class HitStatus(enum.IntEnum):
    """vr_hit.status (VR_HIT_*)."""
    MISS = _capi.VR_HIT_MISS          # the walk left the scene: background
    VOXEL = _capi.VR_HIT_VOXEL        # the walk read a stored voxel
    NEVER = _capi.VR_HIT_NEVER        # the reference's walk would never finish (the render writes 0)
    OUTSIDE = _capi.VR_HIT_OUTSIDE    # the pixel is outside the frame: no ray


# vr_hit, field for field (64 bytes)
HIT_DTYPE = np.dtype([("status", "<u4"), ("color", "<u4"), ("voxel", "<i4", (3,)), ("normal", "<i4", (3,)),
                      ("region", "<i4", (3,)), ("point", "<f4", (3,)), ("reserved", "<u4", (2,))])
assert HIT_DTYPE.itemsize == ctypes.sizeof(_capi.VrHit) == 64


def _ptr(a) -> c_void_p:
    """The address of a CUDA tensor's or a numpy array's first element."""
    return c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)


def _pixel_lists(px, py):
    """px/py of pick and camera_rays as flat arrays: (px, py, n, on_device) -- contiguous CUDA
    tensors when px is one, uint32 numpy arrays otherwise."""
    on_device = hasattr(px, "is_cuda") and px.is_cuda
    if on_device:
        if not (hasattr(py, "is_cuda") and py.is_cuda) or px.device != py.device:
            raise TypeError("px and py must both be CUDA tensors on one device")
        for t in (px, py):
            if t.dtype not in (torch.int32, torch.uint32):
                raise TypeError("px/py must be int32 or uint32 tensors")
        px, py = px.contiguous().reshape(-1), py.contiguous().reshape(-1)
    else:
        px = np.ascontiguousarray(px, dtype=np.uint32).reshape(-1)
        py = np.ascontiguousarray(py, dtype=np.uint32).reshape(-1)
    if px.shape[0] != py.shape[0]:
        raise ValueError("px and py lengths differ")
    return px, py, px.shape[0], on_device


def _records(n: int, dtype: np.dtype, like):
    """The result of a query of n records of `dtype`: beside a CUDA tensor `like`, an (n, words)
    tensor on its device (float32 for rays, int32 for hits); otherwise a zeroed numpy array."""
    if hasattr(like, "is_cuda") and like.is_cuda:
        return torch.empty((n, dtype.itemsize // 4), dtype=torch.float32 if dtype == RAY_DTYPE else torch.int32,
                           device=like.device)
    return np.zeros(n, dtype=dtype)


def pick(scene: DeviceScene, algorithm: RayMarchAlgorithm, camera: Camera, info: VoxelSceneInfo, width: int,
         height: int, px, py, stream=None):
    """vr_pick: the voxel, face and hit point behind pixels (px[i], py[i]) of the width x height
    frame that run_raymarching_kernel renders for the same scene, algorithm, camera and info --
    exactly the hit each pixel is shaded from (y = 0 is the top row).  numpy (or list) px/py
    give a numpy structured array of HIT_DTYPE; CUDA int32/uint32 tensors on the scene's
    device give an (n, 16) int32 CUDA tensor of the same bytes.  `voxel` is what
    DeviceScene.edit takes; `normal` is the reference's shading normal.  Runs on `stream`
    (default: the current stream) and returns when the records are written."""
    args = (scene.handle, int(algorithm), ctypes.byref(camera.raw), f3(info.translation), int(info.scale), int(width),
            int(height))
    px, py, n, dev = _pixel_lists(px, py)
    hits = _records(n, HIT_DTYPE, px)
    if n:
        check(lib().vr_pick(*args, _ptr(px), _ptr(py), n, dev, _ptr(hits), dev, _stream_ptr(stream)), "vr_pick")
    return hits


class TraceOrder(enum.IntEnum):
    """vr_trace_order: which lane walks which ray (the records never depend on it)."""
    AUTO = _capi.VR_TRACE_ORDER_AUTO            # the library's measured choice (include/vr.h)
    GIVEN = _capi.VR_TRACE_ORDER_GIVEN          # lane i walks ray i
    COHERENT = _capi.VR_TRACE_ORDER_COHERENT    # rays sorted on the device by direction and origin cell


# vr_ray, field for field (32 bytes)
RAY_DTYPE = np.dtype([("origin", "<f4", (3,)), ("reserved0", "<u4"), ("direction", "<f4", (3,)), ("reserved1", "<u4")])
assert RAY_DTYPE.itemsize == ctypes.sizeof(_capi.VrRay) == 32


def _rays_numpy(rays) -> np.ndarray:
    """A RAY_DTYPE array from a RAY_DTYPE array or an (n, 6) array of origin and direction."""
    if isinstance(rays, np.ndarray) and rays.dtype == RAY_DTYPE:
        return np.ascontiguousarray(rays).reshape(-1)
    a = np.asarray(rays, dtype=np.float32)
    if a.size == 0:
        return np.zeros(0, dtype=RAY_DTYPE)
    if a.ndim != 2 or a.shape[1] != 6:
        raise ValueError("rays must be a RAY_DTYPE array or an (n, 6) array: origin, direction")
    out = np.zeros(a.shape[0], dtype=RAY_DTYPE)
    out["origin"], out["direction"] = a[:, :3], a[:, 3:]
    return out


def _rays_cuda(rays):
    """An (n, 8) contiguous float32 CUDA tensor, the bytes of vr_ray, from one or from an (n, 6) tensor."""
    if rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] not in (6, 8):
        raise TypeError("rays must be a float32 CUDA tensor of shape (n, 8) or (n, 6)")
    if rays.shape[1] == 6:
        full = torch.zeros((rays.shape[0], 8), dtype=torch.float32, device=rays.device)
        full[:, 0:3], full[:, 4:7] = rays[:, 0:3], rays[:, 3:6]
        rays = full
    return rays.contiguous()


def trace(scene: DeviceScene, algorithm: RayMarchAlgorithm, info: VoxelSceneInfo, rays,
          order: TraceOrder = TraceOrder.AUTO, stream=None):
    """vr_trace: the closest hit of each ray -- the record pick() gives for a pixel, for rays that
    are no pixel of a camera.  The walk starts at the world-space `origin` and runs along
    direction / |direction| (any length); info gives the translation and scale, as for a render.
    A numpy RAY_DTYPE array, or an (n, 6) float array of origin and direction, gives a numpy
    HIT_DTYPE array; a CUDA float32 tensor on the scene's device -- (n, 8), the bytes of vr_ray,
    or (n, 6) -- gives an (n, 16) int32 CUDA tensor of the records' bytes.  `order` changes the
    execution order only, never a record.  A zero, NaN or infinite ray gets the record the
    reference's walk gives it.  Runs on `stream` (default: the current stream) and returns when
    the records are written."""
    args = (scene.handle, int(algorithm), f3(info.translation), int(info.scale))
    dev = hasattr(rays, "is_cuda") and rays.is_cuda
    rays = _rays_cuda(rays) if dev else _rays_numpy(rays)
    n = rays.shape[0]
    hits = _records(n, HIT_DTYPE, rays)
    if n:
        check(lib().vr_trace(*args, _ptr(rays), n, dev, _ptr(hits), dev, int(order), _stream_ptr(stream)), "vr_trace")
    return hits


def shade(scene: DeviceScene, algorithm: RayMarchAlgorithm, info: VoxelSceneInfo, lighting: _capi.VrLighting, rays,
          order: TraceOrder = TraceOrder.AUTO, hits: bool = False, stream=None):
    """vr_shade: the colour a render writes for a pixel whose ray is rays[i] -- lit as the render
    lights it and, with lighting.use_shadows, shadowed by the render's shadow walk; 0 for a miss
    and for a walk the reference would never finish.  shade(camera_rays(...)) of a frame's pixels
    is that frame's render, word for word.  The ray forms are trace()'s.  numpy rays give a uint32
    numpy array of n words (0x00RRGGBB); a CUDA tensor gives an int32 CUDA tensor of shape (n,)
    with the same bits.  hits=True returns (colours, records), the records as trace() returns
    them and from the same walk.  `order` changes the execution order only.  Runs on `stream`
    (default: the current stream) and returns when the outputs are written."""
    args = (scene.handle, int(algorithm), ctypes.byref(lighting), f3(info.translation), int(info.scale))
    dev = hasattr(rays, "is_cuda") and rays.is_cuda
    rays = _rays_cuda(rays) if dev else _rays_numpy(rays)
    n = rays.shape[0]
    colors = torch.empty(n, dtype=torch.int32, device=rays.device) if dev else np.zeros(n, dtype=np.uint32)
    recs = _records(n, HIT_DTYPE, rays) if hits else None
    if n:
        check(lib().vr_shade(*args, _ptr(rays), n, dev, _ptr(colors), _ptr(recs) if hits else None, dev, int(order),
                             _stream_ptr(stream)), "vr_shade")
    return (colors, recs) if hits else colors


class AoApply(enum.IntEnum):
    """vr_ao_apply: what shade_lights(ao=...) scales by the occlusion."""
    AMBIENT = _capi.VR_AO_AMBIENT    # the ambient term only
    ALL = _capi.VR_AO_ALL            # the whole word


AO_OPEN = _capi.VR_AO_OPEN


def occlusion(scene: DeviceScene, hits, stream=None):
    """vr_occlusion: voxel ambient occlusion of hit records -- for each record how open its face is
    at the hit point, 0..255 (AO_OPEN = 255), from the eight voxels around the cell in front of the
    face (include/vr.h has the arithmetic).  Records of pick(), trace(), shade() and shade_lights(),
    or made up: a record that is no VOXEL hit with a unit axis normal is open.  A numpy HIT_DTYPE
    array gives a uint32 numpy array; an (n, 16) int32 CUDA tensor on the scene's device gives an
    int32 CUDA tensor of shape (n,).  Runs on `stream` (default: the current stream) and returns
    when the values are written; no render launch."""
    dev = int(hasattr(hits, "is_cuda") and hits.is_cuda)
    if dev:
        if hits.dtype != torch.int32 or hits.dim() != 2 or hits.shape[1] != 16:
            raise TypeError("hits must be a HIT_DTYPE array or an (n, 16) int32 CUDA tensor")
        hits = hits.contiguous()
        ao = torch.empty(hits.shape[0], dtype=torch.int32, device=hits.device)
    else:
        if not (isinstance(hits, np.ndarray) and hits.dtype == HIT_DTYPE):
            raise TypeError("hits must be a HIT_DTYPE array or an (n, 16) int32 CUDA tensor")
        hits = np.ascontiguousarray(hits).reshape(-1)
        ao = np.zeros(hits.shape[0], dtype=np.uint32)
    if hits.shape[0]:
        check(lib().vr_occlusion(scene.handle, _ptr(hits), hits.shape[0], dev, _ptr(ao), dev, _stream_ptr(stream)),
              "vr_occlusion")
    return ao


def shade_lights(scene: DeviceScene, algorithm: RayMarchAlgorithm, info: VoxelSceneInfo, lights, rays, ambient=None,
                 order: TraceOrder | None = None, hits: bool = False, stream=None, ao=None, ao_apply=None,
                 return_ao: bool = False, reflect=None, bounces: int = 1, mirror=None, atmosphere=None):
    """vr_shade_lights: shade() under several lights and an ambient term, from one primary walk per
    ray.  `lights` is a sequence of VrLighting blocks (at most VR_MAX_LIGHTS, possibly empty), each
    taken exactly as shade() takes its one; `ambient` is three floats or None.  colours[i] is, per
    channel, min(255, the sum of that channel over shade()'s word under each light and the ambient
    term of the hit's stored colour) -- independent of the order of the lights; a miss and a
    primary walk that never ends give 0.  Ray forms, output forms, `order` and hits=True are
    shade()'s.  Runs on `stream` (default: the current stream) and returns when the outputs are
    written.
    ao (a strength 0..255, or None): vr_shade_lights_ao -- the ambient term (ao_apply
    AoApply.AMBIENT, the default) or the whole word (AoApply.ALL) scaled by the factor the strength
    makes of the hit's occlusion(); return_ao=True appends the occlusion values (as occlusion()
    returns them) to the result.  With ao=None the call is vr_shade_lights.
    reflect (a reflectivity 0..255, or None): vr_shade_lights_reflect -- mirror reflections, the
    whole descent on the device: a ray whose hit voxel passes the mirror test bounces (bounce_rays())
    up to `bounces` times (at most MAX_BOUNCES), each depth shaded as the first (lights, ambient, ao),
    and the words are blended from the back, (first * (255 - reflect) + deeper * reflect + 127) // 255
    per channel.  mirror = (mask, value): a voxel reflects when stored colour & mask == value; the
    default (None) is every voxel.  hits and the occlusion values stay those of the first hit.  With
    reflect=None the call is the one above, and bounces and mirror must be left alone.
    atmosphere (an Atmosphere, or None): vr_shade_lights_atmosphere -- at every depth a ray that misses
    shows the sky in its direction (Atmosphere.SKY) and a hit is blended towards the fog's colour by
    the length of its leg (Atmosphere.FOG), as atmosphere_apply() does it, before the depths are
    blended; hits and the occlusion values stay as they are.  With atmosphere=None, or one whose
    flags are 0, the call is the one above."""
    if ao is None and (return_ao or ao_apply is not None):
        raise ValueError("ao_apply and return_ao need ao= (a strength 0..255)")
    if reflect is None and (mirror is not None or int(bounces) != 1):
        raise ValueError("bounces and mirror need reflect= (a reflectivity 0..255)")
    lights = list(lights)
    block = (_capi.VrLighting * max(len(lights), 1))(*lights)
    if ambient is not None and len(ambient) != 3:
        raise ValueError("ambient must be three floats")
    amb = None if ambient is None else f3(ambient)
    args = (scene.handle, int(algorithm), block, len(lights), amb, f3(info.translation), int(info.scale))
    dev = hasattr(rays, "is_cuda") and rays.is_cuda
    rays = _rays_cuda(rays) if dev else _rays_numpy(rays)
    n = rays.shape[0]
    colors = torch.empty(n, dtype=torch.int32, device=rays.device) if dev else np.zeros(n, dtype=np.uint32)
    recs = _records(n, HIT_DTYPE, rays) if hits else None
    tail = (_ptr(rays), n, dev, _ptr(colors), _ptr(recs) if hits else None, dev,
            int(TraceOrder.AUTO if order is None else order), _stream_ptr(stream))
    if reflect is not None or atmosphere is not None:
        strength, apply = int(0 if ao is None else ao), int(AoApply.AMBIENT if ao_apply is None else ao_apply)
        refl = (int(0 if reflect is None else reflect), int(0 if reflect is None else bounces))
        refl += (0, 0) if mirror is None else (int(mirror[0]), int(mirror[1]))
        if any(not 0 <= x < 1 << 32 for x in (strength, apply) + refl):
            raise ValueError("reflect, bounces, mirror, ao and ao_apply must be unsigned 32-bit values")
        values = None
        if return_ao:
            values = torch.empty(n, dtype=torch.int32, device=rays.device) if dev else np.zeros(n, dtype=np.uint32)
        # (the library refuses what it refuses with its message, rays or none)
        if atmosphere is not None:
            check(lib().vr_shade_lights_atmosphere(*args, *tail, strength, apply, _ptr(values) if return_ao else None, *refl,
                                                   ctypes.byref(_atmosphere_raw(atmosphere))), "vr_shade_lights_atmosphere")
        else:
            check(lib().vr_shade_lights_reflect(*args, *tail, strength, apply, _ptr(values) if return_ao else None, *refl),
                  "vr_shade_lights_reflect")
        out = (colors,) + ((recs,) if hits else ()) + ((values,) if return_ao else ())
        return out if len(out) > 1 else colors
    if ao is None:
        if len(lights) > _capi.VR_MAX_LIGHTS or n:     # (the library refuses too many lights, with its message)
            check(lib().vr_shade_lights(*args, *tail), "vr_shade_lights")
        return (colors, recs) if hits else colors
    strength, apply = int(ao), int(AoApply.AMBIENT if ao_apply is None else ao_apply)
    if not 0 <= strength < 1 << 32 or not 0 <= apply < 1 << 32:
        raise ValueError("ao must be a strength 0..255 and ao_apply an AoApply")
    values = None
    if return_ao:
        values = torch.empty(n, dtype=torch.int32, device=rays.device) if dev else np.zeros(n, dtype=np.uint32)
    # (the library refuses too many lights, a strength above 255 and an unknown mode, with its message)
    if len(lights) > _capi.VR_MAX_LIGHTS or strength > 255 or apply not in (0, 1) or n:
        check(lib().vr_shade_lights_ao(*args, *tail, strength, apply, _ptr(values) if return_ao else None),
              "vr_shade_lights_ao")
    out = (colors,) + ((recs,) if hits else ()) + ((values,) if return_ao else ())
    return out if len(out) > 1 else colors


def _tile_order_pixels(width: int, height: int, device):
    """(px, py) of every pixel of the frame as int32 tensors on `device`, 8 x 8 tile by tile (tiles
    row-major, pixels row-major in a tile): the order in which the rays of a frame walk fastest."""
    tw, th = -(-width // 8), -(-height // 8)
    y = torch.arange(th * 8, dtype=torch.int32, device=device).view(th, 1, 8, 1).expand(th, tw, 8, 8).reshape(-1)
    x = torch.arange(tw * 8, dtype=torch.int32, device=device).view(1, tw, 1, 8).expand(th, tw, 8, 8).reshape(-1)
    if tw * 8 != width or th * 8 != height:
        keep = (x < width) & (y < height)
        x, y = x[keep], y[keep]
    return x.contiguous(), y.contiguous()


def render_lights(scene: DeviceScene, algorithm: RayMarchAlgorithm, camera: Camera, info: VoxelSceneInfo, lights,
                  width: int, height: int, ambient=None, stream=None, samples: int = 1, ao=None, ao_apply=None,
                  return_ao: bool = False, reflect=None, bounces: int = 1, mirror=None, atmosphere=None):
    """A width x height frame under several lights and an ambient term: shade_lights() of the
    frame's camera_rays(), as a (height, width) int32 CUDA tensor of 0x00RRGGBB words on the
    scene's device.  The rays are taken in 8 x 8-tile order (row-major rays measured 18-26 %
    slower, profiles/shade/README.md) and the words scattered back to their pixels.  With one light
    and no ambient term it is the frame run_raymarching_kernel renders under that light.
    samples > 1 (2, 4 or 8 per axis): the (samples * width) x (samples * height) frame made the same
    way -- its camera_rays in the 8 x 8-tile order of the fine frame -- and box-filtered by
    resolve().
    ao, ao_apply: shade_lights()'s, for every ray of the frame (of the fine frame with samples > 1).
    return_ao=True returns (frame, values): the occlusion values of the frame's pixels as a
    (height, width) int32 CUDA tensor -- of the fine frame's, (samples * height, samples * width),
    with samples > 1 (they are not filtered).
    reflect, bounces, mirror: shade_lights()'s mirror reflections, for every ray of the frame (of the
    fine frame with samples > 1).
    atmosphere: shade_lights()'s sky and distance fog, for every ray of the frame (of the fine frame
    with samples > 1: the filter then blends sky and voxels along an edge)."""
    samples = int(samples)
    if samples != 1:
        if samples not in (2, 4, 8):
            raise ValueError("samples must be 1, 2, 4 or 8")
        fine = render_lights(scene, algorithm, camera, info, lights, samples * int(width), samples * int(height),
                             ambient=ambient, stream=stream, ao=ao, ao_apply=ao_apply, return_ao=return_ao,
                             reflect=reflect, bounces=bounces, mirror=mirror, atmosphere=atmosphere)
        if return_ao:
            return resolve(fine[0], width, height, samples, stream=stream), fine[1]
        return resolve(fine, width, height, samples, stream=stream)
    device = torch.device(f"cuda:{scene.info()['device']}")
    stream = torch.cuda.current_stream(device) if stream is None else stream
    with torch.cuda.stream(stream):
        px, py = _tile_order_pixels(int(width), int(height), device)
        rays = camera_rays(camera, width, height, px, py, device=device.index, stream=stream)
        words = shade_lights(scene, algorithm, info, lights, rays, ambient=ambient, stream=stream, ao=ao, ao_apply=ao_apply,
                             return_ao=return_ao, reflect=reflect, bounces=bounces, mirror=mirror, atmosphere=atmosphere)
        frame = torch.empty((int(height), int(width)), dtype=torch.int32, device=device)
        frame[py.long(), px.long()] = words[0] if return_ao else words
        if return_ao:
            values = torch.empty((int(height), int(width)), dtype=torch.int32, device=device)
            values[py.long(), px.long()] = words[1]
            return frame, values
    return frame


def aa_fine_words(width: int, rows: int, samples: int) -> int:
    """vr_aa_fine_words: the words of the fine frame behind `rows` rows of a frame `width` wide at
    samples x samples samples per pixel; 0 for arguments render_aa() refuses."""
    if not (0 <= int(width) < 1 << 32 and 0 <= int(rows) < 1 << 32 and 0 <= int(samples) < 1 << 32):
        return 0
    return int(lib().vr_aa_fine_words(int(width), int(rows), int(samples)))


def _resolve_outputs(width: int, rows: int, rgb8, out, device):
    """The outputs of resolve() and render_aa(): (words tensor or None, RGB8 tensor or None)."""
    n = int(width) * int(rows)
    rgb = None
    if rgb8 is not False and rgb8 is not None:
        rgb = torch.empty((int(rows), int(width), 3), dtype=torch.uint8, device=device) if rgb8 is True else rgb8
        if not rgb.is_cuda or rgb.dtype != torch.uint8 or not rgb.is_contiguous() or rgb.numel() < 3 * n:
            raise ValueError(f"rgb8 must be True or a contiguous CUDA uint8 tensor of >= {3 * n} bytes")
    if out is None and rgb is None:
        out = torch.empty((int(rows), int(width)), dtype=torch.int32, device=device)
    if out is not None:
        _require_u32(out, n)
    return out, rgb


def resolve(fine: torch.Tensor, width: int, rows: int, samples: int, rgb8=False, out: torch.Tensor | None = None,
            stream=None):
    """vr_resolve: box-filter the fine frame `fine` -- a contiguous CUDA int32/uint32 tensor of
    (samples * width) x (samples * rows) packed words, row-major: a render, a render_lights frame,
    an assembled multi-GPU frame -- to width x rows pixels: per channel the mean of a pixel's
    samples x samples words, rounded half up; bits 24-31 of a fine word are dropped.  samples is 1,
    2, 4 or 8 per axis.  Returns the words, a (rows, width) int32 tensor (or `out`, filled).
    rgb8=True (or a uint8 tensor to fill): the pixels as RGB8 bytes, (rows, width, 3), R first, as
    pack_rgb8 -- alone when `out` is None, else (out, rgb), both from one read of the fine frame.
    Asynchronous on `stream` (default: the current stream); allocates only the outputs it returns."""
    if not fine.is_cuda or fine.dtype not in (torch.int32, torch.uint32) or not fine.is_contiguous():
        raise TypeError("fine must be a contiguous CUDA int32/uint32 tensor")
    need = int(samples) * int(samples) * int(width) * int(rows)
    if fine.numel() < need:
        raise ValueError(f"fine must hold >= {need} words")
    out, rgb = _resolve_outputs(width, rows, rgb8, out, fine.device)
    with torch.cuda.device(fine.device):
        check(lib().vr_resolve(_ptr(fine), int(width), int(rows), int(samples), None if out is None else _ptr(out),
                               None if rgb is None else _ptr(rgb), _stream_ptr(stream)), "vr_resolve")
    return rgb if out is None else (out if rgb is None else (out, rgb))


def render_aa(scene: DeviceScene, algorithm: RayMarchAlgorithm, camera: Camera, lighting: _capi.VrLighting,
              info: VoxelSceneInfo, width: int, height: int, samples: int, rows=None,
              fine: torch.Tensor | None = None, out: torch.Tensor | None = None, rgb8=False, stream=None):
    """vr_render_aa: the width x height frame at samples x samples (1, 2, 4 or 8 per axis) samples
    per pixel -- run_raymarching_kernel's frame of (samples * width) x (samples * height), rendered
    into `fine` and box-filtered as resolve() does it.  rows = (row_begin, row_end) renders and
    resolves only those rows of the frame (default: all).  `fine`: a CUDA int32/uint32 tensor of
    aa_fine_words(width, row_end - row_begin, samples) words that the caller keeps for the frame
    loop (afterwards it holds the fine rows); allocated here when not given.  `out`, rgb8 and the
    return value are resolve()'s.  An ordinary render launch: a repeated view learns and uses its
    orders.  Asynchronous on `stream` (default: the current stream)."""
    row_begin, row_end = (0, int(height)) if rows is None else (int(rows[0]), int(rows[1]))
    if not 0 <= row_begin <= row_end:
        raise ValueError("rows must be (row_begin, row_end) with 0 <= row_begin <= row_end")
    nrows = row_end - row_begin
    device = torch.device(f"cuda:{scene.info()['device']}")
    words = aa_fine_words(width, nrows, samples)
    if fine is None:
        fine = torch.empty(max(words, 1), dtype=torch.int32, device=device)
    if not fine.is_cuda or fine.dtype not in (torch.int32, torch.uint32) or not fine.is_contiguous():
        raise TypeError("fine must be a contiguous CUDA int32/uint32 tensor")
    out, rgb = _resolve_outputs(width, nrows, rgb8, out, device)
    if nrows == 0 and row_end <= int(height):       # (an empty range does nothing; empty tensors have no address)
        return rgb if out is None else (out if rgb is None else (out, rgb))
    check(lib().vr_render_aa(scene.handle, int(algorithm), ctypes.byref(camera.raw), ctypes.byref(lighting),
                             f3(info.translation), int(info.scale), int(width), int(height), int(samples), row_begin,
                             row_end, _ptr(fine), fine.numel(), None if out is None else _ptr(out),
                             None if rgb is None else _ptr(rgb), _stream_ptr(stream)), "vr_render_aa")
    return rgb if out is None else (out if rgb is None else (out, rgb))


def camera_rays(camera: Camera, width: int, height: int, px, py, device: int = 0, stream=None):
    """vr_camera_rays: the rays a render or pick walks for pixels (px[i], py[i]) of a width x height
    frame (y = 0 is the top row): origin on the image plane, direction origin - eye, not
    normalised, so trace(camera_rays(px, py)) has the bytes of pick(px, py) for pixels inside the
    frame; a pixel outside it gets an all-NaN ray.  numpy (or list) px/py give a numpy RAY_DTYPE
    array; CUDA int32/uint32 tensors give an (n, 8) float32 CUDA tensor of the same bytes."""
    args = (int(device), ctypes.byref(camera.raw), int(width), int(height))
    px, py, n, dev = _pixel_lists(px, py)
    rays = _records(n, RAY_DTYPE, px)
    if n:
        check(lib().vr_camera_rays(*args, _ptr(px), _ptr(py), n, dev, _ptr(rays), dev, _stream_ptr(stream)),
              "vr_camera_rays")
    return rays


MAX_BOUNCES = _capi.VR_MAX_BOUNCES


def bounce_rays(rays, hits, info: VoxelSceneInfo, device: int = 0, stream=None):
    """vr_bounce_rays: the mirror bounce of rays[i] at the hit record hits[i] -- origin the hit point
    back in world units, info.translation + (region * 64 + point) / info.scale, direction the
    incoming one with the sign of the hit normal's axis flipped (not normalised).  A record that is
    no VOXEL hit with a unit axis normal gives an all-NaN ray, which is not harmless to trace: mask
    what you trace by the records' status.  No mirror test is applied.  numpy rays (a RAY_DTYPE
    array or (n, 6)) with a HIT_DTYPE array give a RAY_DTYPE array; CUDA tensors -- float32 (n, 8) or
    (n, 6) rays and (n, 16) int32 records on one device -- give an (n, 8) float32 CUDA tensor there
    (`device` is then not used).  Needs no scene."""
    dev = int(hasattr(rays, "is_cuda") and rays.is_cuda)
    if dev:
        if not (hasattr(hits, "is_cuda") and hits.is_cuda) or hits.device != rays.device:
            raise TypeError("rays and hits must both be CUDA tensors on one device, or both numpy arrays")
        if hits.dtype != torch.int32 or hits.dim() != 2 or hits.shape[1] != 16:
            raise TypeError("hits must be a HIT_DTYPE array or an (n, 16) int32 CUDA tensor")
        rays, hits = _rays_cuda(rays), hits.contiguous()
        device = rays.device.index
    else:
        if not (isinstance(hits, np.ndarray) and hits.dtype == HIT_DTYPE):
            raise TypeError("hits must be a HIT_DTYPE array or an (n, 16) int32 CUDA tensor")
        rays, hits = _rays_numpy(rays), np.ascontiguousarray(hits).reshape(-1)
    n = rays.shape[0]
    if hits.shape[0] != n:
        raise ValueError("rays and hits lengths differ")
    out = _records(n, RAY_DTYPE, rays)
    if n:
        check(lib().vr_bounce_rays(int(device), f3(info.translation), int(info.scale), _ptr(rays), _ptr(hits), n, dev,
                                   _ptr(out), dev, _stream_ptr(stream)), "vr_bounce_rays")
    return out


class Atmosphere:
    """vr_atmosphere: a sky and a linear distance fog, plain data (include/vr.h has the arithmetic).
    zenith, horizon and nadir are the sky's colours (three floats each, 1.0 = 255) straight up,
    level and straight down along `up` (not normalised by the library); a hit's word is blended
    towards fog_color by (distance - fog_start) / (fog_end - fog_start), in world units.  flags is
    Atmosphere.SKY | Atmosphere.FOG: what is applied.  Arguments left None keep
    atmosphere_default()'s values: a daylight sky, up (0, 1, 0), fog off.  `raw` is the VrAtmosphere
    block; changing it in place changes the next call."""
    SKY, FOG = _capi.VR_ATMOS_SKY, _capi.VR_ATMOS_FOG

    def __init__(self, zenith=None, horizon=None, nadir=None, up=None, fog_color=None, fog_start=None, fog_end=None,
                 flags=None):
        self.raw = _capi.VrAtmosphere()
        check(lib().vr_atmosphere_default(ctypes.byref(self.raw)), "vr_atmosphere_default")
        for name, value in (("zenith", zenith), ("horizon", horizon), ("nadir", nadir), ("up", up), ("fog_color", fog_color)):
            if value is not None:
                if len(value) != 3:
                    raise ValueError(f"{name} must be three floats")
                setattr(self.raw, name, f3(value))
        if fog_start is not None:
            self.raw.fog_start = float(fog_start)
        if fog_end is not None:
            self.raw.fog_end = float(fog_end)
        if flags is not None:
            if not 0 <= int(flags) < 1 << 32:
                raise ValueError("flags must be an unsigned 32-bit value")
            self.raw.flags = int(flags)

    @property
    def flags(self) -> int:
        return int(self.raw.flags)


def atmosphere_default() -> Atmosphere:
    """vr_atmosphere_default: a daylight sky with up = (0, 1, 0), fog off, flags Atmosphere.SKY."""
    return Atmosphere()


def _atmosphere_raw(atmosphere) -> _capi.VrAtmosphere:
    if isinstance(atmosphere, Atmosphere):
        return atmosphere.raw
    if isinstance(atmosphere, _capi.VrAtmosphere):
        return atmosphere
    raise TypeError("atmosphere must be an Atmosphere (or a VrAtmosphere block)")


def atmosphere_apply(rays, hits, colors, info: VoxelSceneInfo, atmosphere, device: int = 0, stream=None):
    """vr_atmosphere_apply: colors[i] under the atmosphere -- the sky in the direction of rays[i] where
    hits[i] is a MISS (Atmosphere.SKY), colors[i] blended towards the fog's colour by the distance
    from rays[i]'s origin to the hit point where it is a VOXEL record (Atmosphere.FOG), colors[i]
    itself for everything else.  Records of pick(), trace(), shade() and shade_lights(), or made up.
    numpy rays (a RAY_DTYPE array or (n, 6)) with a HIT_DTYPE array and n colour words give a uint32
    numpy array; CUDA tensors -- float32 (n, 8) or (n, 6) rays, (n, 16) int32 records and an int32
    (n,) tensor on one device -- give an int32 CUDA tensor there (`device` is then not used).  Needs
    no scene."""
    raw = _atmosphere_raw(atmosphere)
    dev = int(hasattr(rays, "is_cuda") and rays.is_cuda)
    if dev:
        for t in (hits, colors):
            if not (hasattr(t, "is_cuda") and t.is_cuda) or t.device != rays.device:
                raise TypeError("rays, hits and colors must all be CUDA tensors on one device, or all numpy arrays")
        if hits.dtype != torch.int32 or hits.dim() != 2 or hits.shape[1] != 16:
            raise TypeError("hits must be a HIT_DTYPE array or an (n, 16) int32 CUDA tensor")
        if colors.dtype not in (torch.int32, torch.uint32) or colors.dim() != 1:
            raise TypeError("colors must be an int32 or uint32 CUDA tensor of shape (n,)")
        rays, hits, colors = _rays_cuda(rays), hits.contiguous(), colors.contiguous()
        device = rays.device.index
        out = torch.empty(colors.shape[0], dtype=torch.int32, device=rays.device)
    else:
        if not (isinstance(hits, np.ndarray) and hits.dtype == HIT_DTYPE):
            raise TypeError("hits must be a HIT_DTYPE array or an (n, 16) int32 CUDA tensor")
        rays, hits = _rays_numpy(rays), np.ascontiguousarray(hits).reshape(-1)
        colors = np.ascontiguousarray(colors, dtype=np.uint32).reshape(-1)
        out = np.zeros(colors.shape[0], dtype=np.uint32)
    n = rays.shape[0]
    if hits.shape[0] != n or colors.shape[0] != n:
        raise ValueError("rays, hits and colors lengths differ")
    if n or raw.flags & ~(_capi.VR_ATMOS_SKY | _capi.VR_ATMOS_FOG):    # (the library refuses unknown flags, with its message)
        check(lib().vr_atmosphere_apply(int(device), ctypes.byref(raw), f3(info.translation), int(info.scale), _ptr(rays),
                                        _ptr(hits), _ptr(colors), n, dev, _ptr(out), dev, _stream_ptr(stream)),
              "vr_atmosphere_apply")
    return out


def band_buffer_words(width: int, height: int, band_rows: int, nranks: int) -> int:
    return int(lib().vr_band_buffer_words(width, height, band_rows, nranks))


def render_bands(scene: DeviceScene, algorithm: RayMarchAlgorithm, camera: Camera, lighting: _capi.VrLighting,
                 info: VoxelSceneInfo, width: int, height: int, band_rows: int, rank: int, nranks: int,
                 out: torch.Tensor, stream=None) -> torch.Tensor:
    """This rank's interleaved row bands (band b -> rank b % nranks), packed."""
    _require_u32(out, band_buffer_words(width, height, band_rows, nranks))
    check(lib().vr_render_bands(scene.handle, int(algorithm), ctypes.byref(camera.raw), ctypes.byref(lighting),
                                f3(info.translation), int(info.scale), int(width), int(height), int(band_rows),
                                int(rank), int(nranks), c_void_p(out.data_ptr()), _stream_ptr(stream)),
          "vr_render_bands")
    return out


def tile_buffer_words(width: int, height: int, band_rows: int, tile_cols: int, nranks: int) -> int:
    return int(lib().vr_tile_buffer_words(width, height, band_rows, tile_cols, nranks))


def deal_stride_default(nranks: int) -> int:
    return int(lib().vr_deal_stride_default(nranks))


def forget_orders(device: int = 0) -> None:
    """Drop the work and lane orders the device learned (vr_forget_orders): the next launch
    renders as a first render of its view."""
    check(lib().vr_forget_orders(int(device)), "vr_forget_orders")


def debug_skip_next_crawl(device: int = 0) -> None:
    """Test hook (vr_debug_skip_next_crawl): the device's next launch skips its crawl pass as
    if its slot had seen the view defer nothing -- for the test of the crawl-skip safety net."""
    check(lib().vr_debug_skip_next_crawl(int(device)), "vr_debug_skip_next_crawl")


def debug_capture_lane_order(device: int = 0) -> None:
    """Test hook (vr_debug_capture_lane_order): the device's next launch that makes a lane order
    keeps a host copy of it and of the walk lengths it was made from."""
    check(lib().vr_debug_capture_lane_order(int(device)), "vr_debug_capture_lane_order")


def debug_lane_order(device: int = 0):
    """Test hook (vr_debug_lane_order): the captured lane order as (info, pcost, perm) -- info
    a dict (LW, rows, gx, gy, block_x, block_y, entry_bytes, seat), pcost a (rows, LW) uint32
    array (primary << 16 | shadow walk lengths), perm a (blocks, block_x * block_y) array of
    block pixels (row * block_x + column), entry 64 q + i the pixel of lane i of wave slot q."""
    import numpy as np
    raw = (ctypes.c_uint32 * 8)()
    check(lib().vr_debug_lane_order(int(device), raw, None, 0, None, 0), "vr_debug_lane_order")
    info = dict(zip(LANE_INFO, (int(x) for x in raw)))
    n = info["block_x"] * info["block_y"]
    blocks = -(-info["LW"] // info["block_x"]) * (-(-info["rows"] // info["block_y"]))
    pcost = np.empty((info["rows"], info["LW"]), dtype=np.uint32)
    perm = np.empty((blocks, n), dtype=np.uint8 if info["entry_bytes"] == 1 else np.uint16)
    check(lib().vr_debug_lane_order(int(device), raw, c_void_p(pcost.ctypes.data), pcost.size,
                                    c_void_p(perm.ctypes.data), perm.nbytes), "vr_debug_lane_order")
    return info, pcost, perm


LANE_INFO = ("LW", "rows", "gx", "gy", "block_x", "block_y", "entry_bytes", "seat")


def debug_work_order(device: int = 0):
    """Test hook (vr_debug_work_order): the captured launch's (cost, order) -- cost a (gy, gx, 2)
    uint32 array, each wave's max(primary) + max(shadow) walk length under the captured lane
    order, order the gx * gy words (row << 16 | column) of the work order made from them.
    Raises VrError when the captured launch made no work order from those costs."""
    import numpy as np
    info, _, _ = debug_lane_order(device)
    check(lib().vr_debug_work_order(int(device), None, 0, None, 0), "vr_debug_work_order")
    cost = np.empty((info["gy"], info["gx"], 2), dtype=np.uint32)
    order = np.empty(info["gy"] * info["gx"], dtype=np.uint32)
    check(lib().vr_debug_work_order(int(device), c_void_p(cost.ctypes.data), cost.size,
                                    c_void_p(order.ctypes.data), order.size), "vr_debug_work_order")
    return cost, order


def debug_lane_order_from(pcost, device: int = 0):
    """Test hook (vr_debug_lane_order_from): perm_kernel run on the caller's (rows, LW) uint32
    walk lengths (primary << 16 | shadow) -> (info, perm, cost), as debug_lane_order and
    debug_work_order return them; whatever the kernel left unwritten is 0xFF bytes."""
    import numpy as np
    pcost = np.ascontiguousarray(pcost, dtype=np.uint32)
    if pcost.ndim != 2:
        raise ValueError("pcost must be a (rows, LW) array")
    rows, LW = pcost.shape
    raw = (ctypes.c_uint32 * 8)()
    check(lib().vr_debug_lane_order_from(int(device), None, LW, rows, raw, None, 0, None, 0), "vr_debug_lane_order_from")
    info = dict(zip(LANE_INFO, (int(x) for x in raw)))
    n = info["block_x"] * info["block_y"]
    blocks = -(-info["LW"] // info["block_x"]) * (-(-info["rows"] // info["block_y"]))
    perm = np.empty((blocks, n), dtype=np.uint8 if info["entry_bytes"] == 1 else np.uint16)
    cost = np.empty((info["gy"], info["gx"], 2), dtype=np.uint32)
    check(lib().vr_debug_lane_order_from(int(device), c_void_p(pcost.ctypes.data), LW, rows, raw,
                                         c_void_p(perm.ctypes.data), perm.nbytes, c_void_p(cost.ctypes.data), cost.size),
          "vr_debug_lane_order_from")
    return info, perm, cost


def debug_work_order_from(cost, columns: int, device: int = 0):
    """Test hook (vr_debug_work_order_from): order_kernel run on the caller's costs (two words
    per tile group, groups in rows of `columns`) -> the order's words (row << 16 | column);
    whatever the kernel left unwritten is 0xFFFFFFFF."""
    import numpy as np
    cost = np.ascontiguousarray(cost, dtype=np.uint32).reshape(-1)
    if cost.size % 2:
        raise ValueError("cost must hold two words per tile group")
    groups = cost.size // 2
    order = np.empty(groups, dtype=np.uint32)
    check(lib().vr_debug_work_order_from(int(device), c_void_p(cost.ctypes.data), int(columns), groups,
                                         c_void_p(order.ctypes.data)), "vr_debug_work_order_from")
    return order


ORDER_USES = ("launches", "lane_orders_made", "lane_order_uses", "work_orders_made", "work_order_uses",
              "crawl_skips", "slots", "lane_block")


def debug_order_uses(device: int = 0) -> dict:
    """Test hook (vr_debug_order_uses): the device's monotonic launch counters as a dict --
    launches, lane_orders_made, lane_order_uses, work_orders_made, work_order_uses,
    crawl_skips, the ring's slots and lane_block = (width, height) in pixels.  Host state
    only: no HIP call."""
    raw = (ctypes.c_uint64 * 8)()
    check(lib().vr_debug_order_uses(int(device), raw), "vr_debug_order_uses")
    d = dict(zip(ORDER_USES, (int(x) for x in raw)))
    d["lane_block"] = (d["lane_block"] >> 16, d["lane_block"] & 0xFFFF)
    return d


def debug_force_in_flight(device: int = 0, on: bool = True) -> None:
    """Test hook (vr_debug_force_in_flight): while on, every launch of the device plans as if
    another stream's launch were running on it; sticky until turned off."""
    check(lib().vr_debug_force_in_flight(int(device), int(bool(on))), "vr_debug_force_in_flight")


LAST_LAUNCH = ("alone", "heavy", "hi", "crawl_rpw", "crawl_grid", "crawl_ran", "records")


def debug_last_launch(device: int = 0) -> dict:
    """Test hook (vr_debug_last_launch): what the device's most recent render launch decided, as
    a dict -- alone, heavy, hi, crawl_rpw, crawl_grid (workgroups), crawl_ran, and records, the
    count the device's last completed crawl pass reported (wait for the launch first).  Host
    state only: no HIP call."""
    raw = (ctypes.c_uint64 * 8)()
    check(lib().vr_debug_last_launch(int(device), raw), "vr_debug_last_launch")
    return dict(zip(LAST_LAUNCH, (int(x) for x in raw)))


def render_tiles(scene: DeviceScene, algorithm: RayMarchAlgorithm, camera: Camera, lighting: _capi.VrLighting,
                 info: VoxelSceneInfo, width: int, height: int, band_rows: int, tile_cols: int, rank: int,
                 nranks: int, out: torch.Tensor, stream=None) -> torch.Tensor:
    """This rank's tiles of the 2-D deal (block j of band b -> rank (j + stride * b) % nranks), packed."""
    _require_u32(out, tile_buffer_words(width, height, band_rows, tile_cols, nranks))
    check(lib().vr_render_tiles(scene.handle, int(algorithm), ctypes.byref(camera.raw), ctypes.byref(lighting),
                                f3(info.translation), int(info.scale), int(width), int(height), int(band_rows),
                                int(tile_cols), int(rank), int(nranks), c_void_p(out.data_ptr()),
                                _stream_ptr(stream)), "vr_render_tiles")
    return out


def assemble_tiles_device(parts: torch.Tensor, frame: torch.Tensor, elem_bytes: int, width: int, height: int,
                          band_rows: int, tile_cols: int, nranks: int, deal_stride: int = 0,
                          stream=None) -> torch.Tensor:
    """vr_assemble_tiles: rank 0's reassembly on the device.  parts: the nranks tile buffers back to back
    (contiguous, elem_bytes per pixel); frame: width x height pixels of elem_bytes (contiguous)."""
    need = tile_buffer_words(width, height, band_rows, tile_cols, nranks) * nranks * elem_bytes
    for name, t, n in (("parts", parts, need), ("frame", frame, width * height * elem_bytes)):
        if not t.is_cuda or not t.is_contiguous() or t.numel() * t.element_size() < n:
            raise ValueError(f"{name} must be a contiguous CUDA tensor of >= {n} bytes")
    check(lib().vr_assemble_tiles(c_void_p(parts.data_ptr()), c_void_p(frame.data_ptr()), int(elem_bytes),
                                  int(width), int(height), int(band_rows), int(tile_cols), int(nranks),
                                  int(deal_stride), _stream_ptr(stream)), "vr_assemble_tiles")
    return frame


def pack_rgb8(words: torch.Tensor, stream=None, out: torch.Tensor | None = None) -> torch.Tensor:
    """writeColorToFramebuffer (Renderer.cuh:1024-1031) on the device: words -> RGB8 bytes
    (into `out`, uint8 of 3 x words.numel(), when given)."""
    rgb = torch.empty(words.numel() * 3, dtype=torch.uint8, device=words.device) if out is None else out
    if rgb.dtype != torch.uint8 or rgb.numel() != words.numel() * 3 or not rgb.is_contiguous():
        raise ValueError("out must be a contiguous uint8 tensor of 3 x words.numel() bytes")
    check(lib().vr_pack_rgb8(c_void_p(words.data_ptr()), c_void_p(rgb.data_ptr()), words.numel(),
                             _stream_ptr(stream)), "vr_pack_rgb8")
    return rgb


@dataclass
class RenderConfig:
    """One BASELINE.json config."""
    name: str
    grid: int
    p_region: float
    p_cluster: float
    p_voxel: float
    seed: int
    width: int
    height: int
    store: StorageType
    algorithm: RayMarchAlgorithm
    gpus: int = 1
    notes: str = ""
    scale: int = field(init=False)

    def __post_init__(self):
        self.scale = 3 * self.grid // 16        # eye at (6s,2s,6s): just outside the grid's x/z faces

    def voxels(self):
        return synth_scene(self.grid, self.p_region, self.p_cluster, self.p_voxel, self.seed)


CONFIGS = {
    "C1": RenderConfig("C1", 64, 1.0, 0.5, 0.10, 0x1, 256, 256, StorageType.HASH_TABLE, RayMarchAlgorithm.ORIGINAL,
                       notes="scene.vox 64^3, hashtable+original (host-CPU plumbing config)"),
    "C2": RenderConfig("C2", 256, 1.0, 0.30, 0.08, 0x256, 1920, 1080, StorageType.VOXEL_CLUSTER_STORE,
                       RayMarchAlgorithm.ORIGINAL, notes="256^3 synthetic, vcs+original"),
    "C3": RenderConfig("C3", 256, 1.0, 0.30, 0.08, 0x256, 1920, 1080, StorageType.VOXEL_CLUSTER_STORE,
                       RayMarchAlgorithm.LONGEST_AXIS, notes="256^3 synthetic, vcs+longestaxis"),
    "C4": RenderConfig("C4", 512, 1.0, 1.0, 0.15, 0x512, 1920, 1080, StorageType.HASH_TABLE,
                       RayMarchAlgorithm.ORIGINAL, notes="512^3 dense, hashtable+original"),
    "C5": RenderConfig("C5", 1024, 0.35, 0.05, 0.25, 0x1024, 3840, 2160, StorageType.VOXEL_CLUSTER_STORE,
                       RayMarchAlgorithm.ORIGINAL, gpus=8, notes="1024^3 sparse, vcs+original, 8-GPU tiles"),
}
