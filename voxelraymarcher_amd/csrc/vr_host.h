// vr_host.h -- what the host translation units of libvr.so share (vr_host.cpp, vr_scene.cpp,
// vr_scene_io.cpp, vr_launch.cpp, vr_query_api.cpp, vr_aa_api.cpp).  Private: nothing declared here is exported.
// (vr_staging.h, beside it: the staging buffers of the entry points that take host or device arrays.)
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "vr.h"
#include "vr_internal.h"

#pragma GCC visibility push(hidden)

namespace vr {

inline int fail(int code, const std::string& msg) { return set_error(code, msg); }
inline int hip_fail(hipError_t e, const char* what) {
    return fail(VR_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// Nothing of `who` (an entry point, as its messages name it) can be captured into a HIP graph:
// it waits for the stream, allocates, or keeps host-side state that a replay would not redo.
// Called before anything is enqueued or allocated.
inline int refuse_capture(hipStream_t st, const char* who) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    const hipError_t e = hipStreamIsCapturing(st, &cap);
    if (e != hipSuccess) return hip_fail(e, "hipStreamIsCapturing");
    if (cap != hipStreamCaptureStatusNone)
        return fail(VR_E_INVALID, std::string(who) + " cannot be captured into a HIP graph (stream is capturing)");
    return VR_OK;
}

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

// FNV-1a over n bytes, continuing from h (kFnvBasis to start).
constexpr uint64_t kFnvBasis = 1469598103934665603ull;
inline uint64_t fnv1a(uint64_t h, const void* p, size_t n) {
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
};

}  // namespace vr

struct vr_scene {
    // a process-unique id (the learned orders' view key: a later scene may reuse a freed
    // scene's address), drawn by vr_scene.cpp
    const uint64_t serial;
    explicit vr_scene(uint64_t id) : serial(id) {}
    // bumped by every successful non-empty vr_scene_edit: with `serial`, the identity of the
    // scene's CONTENT (which pixels a view defers depends on it; vr_launch.cpp view_key).
    // vr_scene_paint does not bump it: a recolour changes no deferral and no walk length
    uint64_t revision = 0;
    int device = 0;
    vr_store store = VR_STORE_VCS;
    uint32_t D = 1;
    int32_t min_coord = 0;
    uint32_t n_regions = 0;
    uint64_t n_voxels = 0;
    vr::DevBuf region_slot, vcs_mask, vcs_vals, ht_meta, ht_slots;
    vr::DevBuf vcs_cbits;   // derived (not part of vr_scene_digest): cluster-existence bits per region
    vr::DevBuf ht_filter;   // derived (not part of vr_scene_digest): cuckoo key-presence bits per region
    // vr_scene_paint's two result words on the device (vr_internal.h launch_paint_check): made by
    // the scene's first paint, kept for the next ones, freed with the scene; no part of the image
    uint32_t* paint_stat = nullptr;
    uint64_t device_bytes() const {
        return region_slot.bytes + vcs_mask.bytes + vcs_vals.bytes + ht_meta.bytes + ht_slots.bytes + vcs_cbits.bytes +
               ht_filter.bytes;
    }
};

namespace vr {

// vr_scene.cpp
KScene kscene(const vr_scene* s);
int build_scene(int device, vr_store store, const int32_t* xyz, const uint32_t* rgb, size_t n, bool on_device,
                vr_build mode, void* stream, vr_scene** out);

// vr_launch.cpp: the camera and frame size of a view (v.W, v.H, v.LW; nothing else is written),
// its lighting block (L, LC, LP, Lr, L_fast, Lw, L_order, L_cls, L_unit, L_eq and the two flags;
// nothing else is written), and the whole view of a render (zeroed first; the launch's rows and
// tile deal are the caller's)
void view_camera(KView& v, const vr_camera* cam, uint32_t width, uint32_t height);
void view_lighting(KView& v, const vr_lighting* lit);
int make_view(const vr_scene* s, const vr_camera* cam, const vr_lighting* lit, const float translation[3],
              uint32_t scale, uint32_t width, uint32_t height, KView& v);

// vr_scene_io.cpp: a scene file's voxels (.vxb or .vox CSV, read and parsed once)
struct VoxParse {
    std::vector<int32_t> xyz;
    std::vector<uint32_t> rgb;
};
int read_voxels(const char* path, VoxParse& out);

}  // namespace vr

#pragma GCC visibility pop
