// vr_trace.hip -- the coherent execution order of vr_trace (include/vr.h): a 64-bit key per ray
// and a stable radix sort of (key, ray index); trace_kernel (vr_query.hip) then walks ray
// idx[i] in lane i, so the lanes of a wave start near each other and head the same way.  The
// order decides only which lane walks which ray: no record depends on it.
//
// Key, most significant first (kDirBits + 3 * cb + 3 bits in all, the sort's end bit):
//   3 bits        the signs of the normalised direction (x, y, z: 1 = negative)
//   3 * cb bits   the Morton code of the origin's cell: the scene-space origin
//                 (origin - translation) * scale at 8-voxel (cluster) granularity, relative to the
//                 scene's frame and clamped to it (a ray that starts outside lands on a face; a NaN
//                 origin in cell 0), cb = the bits of 8 * D - 1, at most 15 (a larger frame drops
//                 the cell's low bits)
//   16 bits       the direction's cube-map cell: the dominant axis (2 bits) and the Morton code
//                 of the two other components over the dominant one, 7 bits each
// Rays of one origin (a camera's) are ordered by direction alone, which is what an 8x8 pixel
// tile does; scattered origins (bounce rays) are grouped by cell first.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>   // (rocprim's headers call memset)

#include <rocprim/rocprim.hpp>

#include "vr_internal.h"

namespace vr {
namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kDirBits = 16, kMaxCellBits = 15;

// bits 0..14 of v spread to every third bit
__device__ __forceinline__ uint64_t spread3(uint32_t v) {
    uint64_t x = v & 0x7FFFu;
    x = (x | (x << 32)) & 0x001F00000000FFFFull;
    x = (x | (x << 16)) & 0x001F0000FF0000FFull;
    x = (x | (x << 8)) & 0x100F00F00F00F00Full;
    x = (x | (x << 4)) & 0x10C30C30C30C30C3ull;
    x = (x | (x << 2)) & 0x1249249249249249ull;
    return x;
}
// bits 0..6 of v spread to every second bit
__device__ __forceinline__ uint32_t spread2(uint32_t v) {
    uint32_t x = v & 0x7Fu;
    x = (x | (x << 4)) & 0x0F0Fu;
    x = (x | (x << 2)) & 0x3333u;
    x = (x | (x << 1)) & 0x5555u;
    return x;
}
// t in [-1, 1] (or NaN: 0) -> 0..127
__device__ __forceinline__ uint32_t quant7(float t) {
    const float q = fminf(fmaxf((t + 1.0f) * 64.0f, 0.0f), 127.0f);   // fmaxf(NaN, 0) = 0
    return (uint32_t)(int32_t)q;
}

__global__ __launch_bounds__(kThreads) void trace_keys_kernel(const float4* __restrict__ rays, uint32_t n, float tx,
                                                              float ty, float tz, float scale, float lo, float top,
                                                              uint32_t cell_bits, uint32_t cell_drop,
                                                              uint64_t* __restrict__ keys, uint32_t* __restrict__ idx) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float4 a = rays[(size_t)i * 2u], b = rays[(size_t)i * 2u + 1u];
    // the origin's cluster cell in the frame [lo, lo + top] (clusters), clamped; NaN -> 0
    const float so[3] = {scale * (a.x - tx), scale * (a.y - ty), scale * (a.z - tz)};
    uint32_t cell[3];
    for (int k = 0; k < 3; ++k) {
        const float c = fminf(fmaxf(floorf(so[k] * 0.125f) - lo, 0.0f), top);
        cell[k] = (uint32_t)c >> cell_drop;        // (c is in [0, top], top < 2^32)
    }
    const uint64_t morton = spread3(cell[0]) << 2 | spread3(cell[1]) << 1 | spread3(cell[2]);
    // the direction: signs, dominant axis, the other two components over it (the order of a
    // scaled direction is the order of the unit one, so no normalisation is needed for a key)
    const float d[3] = {b.x, b.y, b.z};
    const uint32_t signs = (d[0] < 0.0f ? 4u : 0u) | (d[1] < 0.0f ? 2u : 0u) | (d[2] < 0.0f ? 1u : 0u);
    const float ax = fabsf(d[0]), ay = fabsf(d[1]), az = fabsf(d[2]);
    const uint32_t dom = (ax >= ay && ax >= az) ? 0u : (ay >= az ? 1u : 2u);
    const float m = dom == 0u ? d[0] : (dom == 1u ? d[1] : d[2]);
    const float p = dom == 0u ? d[1] : d[0], q = dom == 2u ? d[1] : d[2];
    const uint32_t dir = dom << 14 | spread2(quant7(p / m)) << 1 | spread2(quant7(q / m));
    keys[i] = ((uint64_t)signs << (3u * cell_bits) | morton) << kDirBits | dir;
    idx[i] = i;
}

}  // namespace

hipError_t trace_order(const KScene& s, const KView& v, const void* rays, uint32_t n, hipStream_t stream,
                       void** scratch, const uint32_t** idx) {
    *scratch = nullptr;
    *idx = nullptr;
    if (n == 0) return hipSuccess;
    // the frame in clusters: [8 * min_coord, 8 * (min_coord + D)) on every axis
    const uint64_t clusters = (uint64_t)std::max<uint32_t>(s.D, 1u) * 8u;
    uint32_t bits = 0;
    while (bits < 32u && ((clusters - 1u) >> bits) != 0u) ++bits;
    bits = std::max(bits, 1u);
    const uint32_t cell_bits = std::min(bits, kMaxCellBits), cell_drop = bits - cell_bits;
    const unsigned end_bit = kDirBits + 3u * cell_bits + 3u;
    // one allocation: keys in / out, indices in / out, the sort's temporary (256-byte aligned parts)
    auto up = [](size_t b) { return (b + 255u) & ~(size_t)255u; };
    const size_t kb = up((size_t)n * sizeof(uint64_t)), ib = up((size_t)n * sizeof(uint32_t));
    size_t sort_bytes = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, sort_bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                             (const uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n, 0u, end_bit, stream);
    if (e != hipSuccess) return e;
    char* base = nullptr;
    e = hipMalloc((void**)&base, 2u * kb + 2u * ib + std::max<size_t>(sort_bytes, 1u));
    if (e != hipSuccess) return e;
    uint64_t *key_a = (uint64_t*)base, *key_b = (uint64_t*)(base + kb);
    uint32_t *idx_a = (uint32_t*)(base + 2u * kb), *idx_b = (uint32_t*)(base + 2u * kb + ib);
    void* sort_tmp = base + 2u * kb + 2u * ib;
    hipLaunchKernelGGL(trace_keys_kernel, dim3((n + kThreads - 1u) / kThreads), dim3(kThreads), 0, stream,
                       static_cast<const float4*>(rays), n, v.translation[0], v.translation[1], v.translation[2], v.scale_f,
                       (float)s.min_coord * 8.0f, (float)std::min<uint64_t>(clusters - 1u, 0xFFFFFF00u), cell_bits,
                       cell_drop, key_a, idx_a);
    e = hipGetLastError();
    if (e == hipSuccess)
        e = rocprim::radix_sort_pairs(sort_tmp, sort_bytes, (const uint64_t*)key_a, key_b, (const uint32_t*)idx_a, idx_b,
                                      (size_t)n, 0u, end_bit, stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(stream);
        (void)hipFree(base);
        return e;
    }
    *scratch = base;
    *idx = idx_b;
    return hipSuccess;
}

}  // namespace vr
