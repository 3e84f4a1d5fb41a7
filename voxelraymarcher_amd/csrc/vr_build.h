// vr_build.h -- the GPU scene builder (vr_build.hip) and the in-place edit (vr_edit.hip),
// used by vr_scene.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

namespace vr {

// Device buffers of one scene (owned by the caller afterwards); layouts as in
// vr_internal.h, identical to the host builder's.
struct GpuScene {
    void* region_slot = nullptr; uint64_t region_slot_bytes = 0;
    void* vcs_mask = nullptr;    uint64_t vcs_mask_bytes = 0;
    void* vcs_vals = nullptr;    uint64_t vcs_vals_bytes = 0;
    void* ht_meta = nullptr;     uint64_t ht_meta_bytes = 0;
    void* ht_slots = nullptr;    uint64_t ht_slots_bytes = 0;
    uint32_t D = 1;
    int32_t min_coord = 0;
    uint32_t n_regions = 0;
    uint64_t n_voxels = 0;
};

// Build from device-resident voxels (xyz: 3n int32, rgb: n colours) on `stream`.
// 0 = OK; -1 invalid input, -2 HIP error, -5 build failure (message in err).
// On failure the buffers already allocated in `out` are the caller's to free.
int build_scene_gpu(int store, const int32_t* xyz, const uint32_t* rgb, uint64_t n, hipStream_t stream,
                    GpuScene& out, std::string& err);

// Cuckoo tables an edit keeps: a region whose byte in `changed` (one per grid region of the
// frame) is 0 has the key set it had in the old image, and its tables are copied from there
// instead of being built again.
struct CuckooReuse {
    const uint8_t* changed;
    const uint32_t* region_slot;
    const void* ht_meta;
    const void* ht_slots;
};

// Step 5 of the build (vr_build.hip's header comment): the scene image of the frame
// (out.D, out.min_coord, set by the caller) from m sorted unique keys; the colour of key j
// is rgb[uidx[j]], or rgb[j] when uidx is null.  Returns as build_scene_gpu does, after
// the stream has drained.
int emit_scene_gpu(int store, const uint64_t* ukey, const uint32_t* uidx, const uint32_t* rgb, uint64_t m,
                   hipStream_t stream, GpuScene& out, std::string& err, const CuckooReuse* reuse = nullptr);

// The image of a scene as the kernels of vr_edit.hip read it.
struct GpuImage {
    int store;
    uint32_t D;
    int32_t min_coord;
    uint32_t n_regions;
    uint64_t n_voxels;
    const void *region_slot, *vcs_mask, *vcs_vals, *ht_meta, *ht_slots, *ht_filter;
};

// vr_scene_edit's device work (vr_edit.hip): the image of `old` with n device-resident edits
// applied, as a from-scratch build of the edited voxel set in old's frame would make it.
// Returns as build_scene_gpu does; -1 with `err` naming the first edit whose colour is
// neither below 2^24 nor VR_VOXEL_REMOVE, or whose region lies outside the frame.
int edit_scene_gpu(const GpuImage& old, const int32_t* xyz, const uint32_t* rgb, uint64_t n, hipStream_t stream,
                   GpuScene& out, std::string& err);

// vr_scene_voxels' device work: the image's voxels in region order, then key order, as world
// coordinates (xyz: 3 * n_voxels int32) and colours (rgb: n_voxels), device buffers.
int export_scene_gpu(const GpuImage& img, int32_t* xyz, uint32_t* rgb, hipStream_t stream, std::string& err);

}  // namespace vr
