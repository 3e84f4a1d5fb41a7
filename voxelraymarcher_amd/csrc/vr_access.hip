// vr_access.hip -- voxel access by coordinate: vr_scene_lookup's kernel and the three kernels of
// vr_scene_paint.  One lane per query; everything rests on locate(), which finds
// the value word of a world voxel in the live image of either store (vr_locate.h).
#include "vr_locate.h"

namespace vr {
namespace {

template <int STORE>
__global__ void lookup_kernel(KScene s, const int32_t* __restrict__ xyz, uint32_t n, uint32_t* __restrict__ rgb) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t* q = xyz + (size_t)i * 3u;
    const uint32_t* p = locate<STORE>(s, q[0], q[1], q[2]);
    rgb[i] = p ? *p : 0xFFFFFFFFu;                               // VR_VOXEL_ABSENT
}

// Paint, before any write: stat[0] = the first index whose colour is not below 2^24 (atomic min),
// stat[1] -= 1 per edit whose voxel is not stored (one atomic per wave).  Both start at
// 0xFFFFFFFF (one memset), so the absent count is 0xFFFFFFFF - stat[1].
template <int STORE>
__global__ void paint_check_kernel(KScene s, const int32_t* __restrict__ xyz, const uint32_t* __restrict__ rgb,
                                   uint32_t n, uint32_t* __restrict__ stat) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool gone = false;
    if (i < n) {
        if (rgb[i] > 0xFFFFFFu) atomicMin(&stat[0], i);
        const int32_t* q = xyz + (size_t)i * 3u;
        gone = locate<STORE>(s, q[0], q[1], q[2]) == nullptr;
    }
    const uint64_t votes = __ballot(gone);
    if (votes != 0ull && (threadIdx.x & 63u) == 0u) atomicSub(&stat[1], (uint32_t)__popcll(votes));
}

// Paint, last edit wins without a sort.  Tag: every edit of a stored voxel raises the voxel's
// value word to 0x80000000 | i with an atomic max -- a tag exceeds every colour (< 2^24) and
// every smaller index's tag (n < 2^31), so the word ends as the tag of the LAST edit of that
// voxel.  Resolve (the next kernel): edit i stores rgb[i] iff the word is its own tag; every
// other edit of the voxel reads another edit's tag or the winner's colour, neither its own tag.
template <int STORE>
__global__ void paint_tag_kernel(KScene s, const int32_t* __restrict__ xyz, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t* q = xyz + (size_t)i * 3u;
    uint32_t* p = const_cast<uint32_t*>(locate<STORE>(s, q[0], q[1], q[2]));
    if (p) atomicMax(p, 0x80000000u | i);
}

template <int STORE>
__global__ void paint_resolve_kernel(KScene s, const int32_t* __restrict__ xyz, const uint32_t* __restrict__ rgb,
                                     uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t* q = xyz + (size_t)i * 3u;
    uint32_t* p = const_cast<uint32_t*>(locate<STORE>(s, q[0], q[1], q[2]));
    if (p && __atomic_load_n(p, __ATOMIC_RELAXED) == (0x80000000u | i)) __atomic_store_n(p, rgb[i], __ATOMIC_RELAXED);
}

inline dim3 lanes(uint32_t n) { return dim3((n + 255u) / 256u); }

}  // namespace

hipError_t launch_lookup(int store, const KScene& s, const int32_t* xyz, uint32_t n, uint32_t* rgb, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (store == STORE_VCS) hipLaunchKernelGGL(lookup_kernel<STORE_VCS>, lanes(n), dim3(256), 0, stream, s, xyz, n, rgb);
    else hipLaunchKernelGGL(lookup_kernel<STORE_HASH>, lanes(n), dim3(256), 0, stream, s, xyz, n, rgb);
    return hipGetLastError();
}

hipError_t launch_paint_check(int store, const KScene& s, const int32_t* xyz, const uint32_t* rgb, uint32_t n,
                              uint32_t* stat, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(stat, 0xFF, 2 * sizeof(uint32_t), stream);
    if (e != hipSuccess || n == 0) return e;
    if (store == STORE_VCS)
        hipLaunchKernelGGL(paint_check_kernel<STORE_VCS>, lanes(n), dim3(256), 0, stream, s, xyz, rgb, n, stat);
    else
        hipLaunchKernelGGL(paint_check_kernel<STORE_HASH>, lanes(n), dim3(256), 0, stream, s, xyz, rgb, n, stat);
    return hipGetLastError();
}

hipError_t launch_paint_apply(int store, const KScene& s, const int32_t* xyz, const uint32_t* rgb, uint32_t n,
                              hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (store == STORE_VCS) {
        hipLaunchKernelGGL(paint_tag_kernel<STORE_VCS>, lanes(n), dim3(256), 0, stream, s, xyz, n);
        hipLaunchKernelGGL(paint_resolve_kernel<STORE_VCS>, lanes(n), dim3(256), 0, stream, s, xyz, rgb, n);
    } else {
        hipLaunchKernelGGL(paint_tag_kernel<STORE_HASH>, lanes(n), dim3(256), 0, stream, s, xyz, n);
        hipLaunchKernelGGL(paint_resolve_kernel<STORE_HASH>, lanes(n), dim3(256), 0, stream, s, xyz, rgb, n);
    }
    return hipGetLastError();
}

}  // namespace vr
