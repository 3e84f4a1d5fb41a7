// vr_util.hip -- the small kernels around the march: a scene's cluster-existence bits and
// hash filter (made once per build or edit), the RGB8 pack and the 2-D tile deal's reassembly.
#include "vr_device.h"

namespace vr {
namespace {

// KScene::vcs_cbits: thread (r, w) ORs the existence of cluster slots 32w..32w+31 of
// region r (a present cluster's record has an index in every word, vr_internal.h)
__global__ void cluster_bits_kernel(const uint2* __restrict__ mask, uint32_t n_regions, uint32_t* __restrict__ cbits) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_regions * 16u) return;
    const uint2* m = mask + (size_t)(t >> 4) * 8192u + (size_t)(t & 15u) * 32u * 16u;
    uint32_t b = 0;
    for (uint32_t k = 0; k < 32u; ++k) b |= (m[k * 16u].y != kNone ? 1u : 0u) << k;
    cbits[t] = b;
}

// KScene::ht_filter: workgroup r sets the presence bit of every key in region r's two tables
// (keys are local generate3DPoint keys: x, y, z < 64)
__global__ void hash_filter_kernel(const uint4* __restrict__ meta, const uint2* __restrict__ slots,
                                   uint32_t* __restrict__ filter) {
    using F = Ctx<STORE_VCS, false, kTileBudget>;
    const uint4 m = meta[blockIdx.x];
    uint32_t* f = filter + (size_t)blockIdx.x * kHashFilterWords;
    for (uint32_t i = threadIdx.x; i < 2u * m.y; i += blockDim.x) {
        const uint32_t k = slots[m.x + i].x;
        if (k == kEmpty) continue;
        const uint32_t x = (k >> 20) & 63u, y = (k >> 10) & 63u, z = k & 63u;
        atomicOr(&f[F::word_index(x, y, z)], 1u << (F::word_bit5(y, z) & 31u));
    }
}

__global__ void pack_rgb8_kernel(const uint32_t* __restrict__ w, uint8_t* __restrict__ rgb, uint64_t n) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t c = w[i];
    rgb[3 * i + 0] = (uint8_t)(c >> 16);
    rgb[3 * i + 1] = (uint8_t)((c >> 8) & 0xFFu);
    rgb[3 * i + 2] = (uint8_t)(c & 0xFFu);
}

// Rank 0's reassembly of the 2-D tile deal (vr_internal.h TileLayout): one thread per frame
// pixel reads its owner's local pixel -- the inverse of pixel_ray's column map -- and copies
// E bytes.  (The gathered buffers are read once and the frame written once: HBM-bound.)
template <int E>
__global__ void assemble_tiles_kernel(const uint8_t* __restrict__ parts, uint8_t* __restrict__ frame, TileLayout t) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)t.W * t.H) return;
    const uint32_t y = (uint32_t)(i / t.W), x = (uint32_t)(i - (uint64_t)y * t.W);
    const uint32_t b = y / t.band_rows, j = x / t.tile_cols, in_blk = x - j * t.tile_cols;
    const uint32_t rank = (j + t.stride * (b % t.R)) % t.R;
    const uint64_t lx = (uint64_t)(j / t.R) * t.tile_cols + in_blk;
    const uint64_t src = (uint64_t)rank * t.rank_words + (uint64_t)y * t.LW + lx;
#pragma unroll
    for (int k = 0; k < E; ++k) frame[i * E + k] = parts[src * E + k];
}

}  // namespace

hipError_t launch_cluster_bits(const uint2* vcs_mask, uint32_t n_regions, uint32_t* cbits, hipStream_t stream) {
    if (n_regions == 0) return hipSuccess;
    const uint32_t threads = n_regions * 16u;
    hipLaunchKernelGGL(cluster_bits_kernel, dim3((threads + 255u) / 256u), dim3(256), 0, stream, vcs_mask, n_regions,
                       cbits);
    return hipGetLastError();
}

hipError_t launch_assemble_tiles(const void* parts, void* frame, uint32_t elem_bytes, const TileLayout& t,
                                 hipStream_t stream) {
    const uint64_t n = (uint64_t)t.W * t.H;
    if (n == 0) return hipSuccess;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    const uint8_t* p = static_cast<const uint8_t*>(parts);
    uint8_t* f = static_cast<uint8_t*>(frame);
    switch (elem_bytes) {
    case 1: hipLaunchKernelGGL(assemble_tiles_kernel<1>, grid, block, 0, stream, p, f, t); break;
    case 2: hipLaunchKernelGGL(assemble_tiles_kernel<2>, grid, block, 0, stream, p, f, t); break;
    case 3: hipLaunchKernelGGL(assemble_tiles_kernel<3>, grid, block, 0, stream, p, f, t); break;
    default: hipLaunchKernelGGL(assemble_tiles_kernel<4>, grid, block, 0, stream, p, f, t); break;
    }
    return hipGetLastError();
}

hipError_t launch_hash_filter(const uint4* ht_meta, const uint2* ht_slots, uint32_t n_regions, uint32_t* filter,
                              hipStream_t stream) {
    if (n_regions == 0) return hipSuccess;
    hipLaunchKernelGGL(hash_filter_kernel, dim3(n_regions), dim3(256), 0, stream, ht_meta, ht_slots, filter);
    return hipGetLastError();
}

hipError_t launch_pack_rgb8(const uint32_t* words, uint8_t* rgb, uint64_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(pack_rgb8_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, words, rgb, n);
    return hipGetLastError();
}

}  // namespace vr
