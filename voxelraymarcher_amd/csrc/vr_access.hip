// vr_access.hip -- voxel access by coordinate: vr_scene_lookup's kernel and the three kernels of
// vr_scene_paint.  One lane per query; everything rests on locate(), which finds
// the value word of a world voxel in the live image of either store.
#include "vr_device.h"

namespace vr {
namespace {

using F = Ctx<STORE_VCS, false, kTileBudget>;   // (for its static arithmetic: word_index, word_bit5)

// The word that holds the colour of world voxel (x, y, z) -- an entry of vcs_vals, or the value
// half of a cuckoo slot -- or null when the voxel is not stored: its 64^3 region outside the
// frame, a null region, an absent cluster, an absent key.  Set membership in the voxel set
// vr_scene_voxels returns: a world coordinate always has local coordinates in [0, 64), so none
// of the walks' out-of-region lookups (vr_device.h lookup_aliased, wrapped keys) exists here.
template <int STORE>
__device__ __forceinline__ const uint32_t* locate(const KScene& s, int32_t x, int32_t y, int32_t z) {
    // region = floor(c / 64), tested against the frame as Ctx::in_scene does (unsigned wrap:
    // any int32 coordinate gives a region in [-2^25, 2^25), far from wrapping back into D <= 1024)
    const uint32_t mc = (uint32_t)s.min_coord;
    const uint32_t ux = (uint32_t)(x >> 6) - mc, uy = (uint32_t)(y >> 6) - mc, uz = (uint32_t)(z >> 6) - mc;
    if (ux >= s.D || uy >= s.D || uz >= s.D) return nullptr;
    const uint32_t r = s.region_slot[ux + uy * s.D + uz * s.D * s.D];
    if (r == kNone) return nullptr;
    const uint32_t lx = (uint32_t)x & 63u, ly = (uint32_t)y & 63u, lz = (uint32_t)z & 63u;
    const uint32_t w = F::word_index(lx, ly, lz), bit = F::word_bit5(ly, lz) & 31u;
    if (STORE == STORE_VCS) {
        const uint2 m = s.vcs_mask[(size_t)r * 8192u + w];      // an absent cluster's words are {0, kNone}
        if (!((m.x >> bit) & 1u)) return nullptr;
        return s.vcs_vals + (m.y + __popc(m.x & ((1u << bit) - 1u)));
    }
    if (!((s.ht_filter[(size_t)r * kHashFilterWords + w] >> bit) & 1u)) return nullptr;
    const uint32_t key = (lx << 20) | (ly << 10) | lz;          // generate3DPoint
    const uint4 m = s.ht_meta[r];                                // {base, M, prime, offset}
    const uint2* e = s.ht_slots + m.x + hash1(key, m.w) % m.y;
    if (e->x != key) e = s.ht_slots + m.x + m.y + hash2(key, m.z) % m.y;
    if (e->x != key) return nullptr;                             // (a filter bit without its key: never, by construction)
    return &e->y;
}

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
