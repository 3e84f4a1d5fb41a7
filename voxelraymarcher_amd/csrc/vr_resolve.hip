// vr_resolve.hip -- vr_resolve's kernel (include/vr.h): the box filter that turns a
// fine frame of (S * W) x (S * rows) packed words into W x rows resolved pixels, as packed words,
// as RGB8, or as both from one read.  Every fine word is loaded exactly once; nothing else is read,
// no LDS, no atomics.  The arithmetic is vr_resolve_math.h's.
#include <hip/hip_runtime.h>

#include "vr_internal.h"
#include "vr_resolve_math.h"

namespace vr {
namespace {

// One workgroup row of 256 lanes covers 256 items of a pixel row; blockIdx.y strides over the
// pixel rows (no division).  VEC (chosen on the host for the whole launch, so wave-uniform): 16-byte
// loads -- S = 2: an item is two pixels, one uint4 from each of the two fine rows; S = 4: an item
// is one pixel, one uint4 per fine row; S = 8: one pixel, two uint4 per fine row.  It needs a
// 16-byte aligned `fine` and, at S = 2, an even W (the row pitch S * W * 4 bytes is then a
// multiple of 16 and no item straddles a row's end).  Otherwise an item is one pixel read with
// S * S one-word loads.  No lane loads outside its own S x S (S = 2 VEC: 4 x 2) block, so none
// reads past its row or past the frame.
template <int S, bool RGB8, bool VEC>
__global__ __launch_bounds__(256) void resolve_kernel(const uint32_t* __restrict__ fine, uint32_t W, uint32_t rows,
                                                       uint32_t* __restrict__ out, uint8_t* __restrict__ rgb) {
    constexpr uint32_t PX = (VEC && S == 2) ? 2u : 1u;      // pixels per item
    constexpr uint32_t SH = ResolveShift<S>::value;
    const uint32_t x = (blockIdx.x * 256u + threadIdx.x) * PX;
    if (x >= W) return;
    const size_t pitch = (size_t)S * W;
    for (uint32_t y = blockIdx.y; y < rows; y += gridDim.y) {
        const uint32_t* p = fine + (size_t)y * S * pitch + (size_t)x * S;
        uint32_t w[PX];
        if constexpr (VEC && S == 2) {
            const uint4 a = *reinterpret_cast<const uint4*>(p);
            const uint4 b = *reinterpret_cast<const uint4*>(p + pitch);
            ResolveSum s0 = {0u, 0u}, s1 = {0u, 0u};
            resolve_add(s0, a.x), resolve_add(s0, a.y), resolve_add(s0, b.x), resolve_add(s0, b.y);
            resolve_add(s1, a.z), resolve_add(s1, a.w), resolve_add(s1, b.z), resolve_add(s1, b.w);
            w[0] = resolve_pack(s0, SH);
            w[1] = resolve_pack(s1, SH);
        } else if constexpr (VEC) {
            ResolveSum s = {0u, 0u};
#pragma unroll
            for (int j = 0; j < S; ++j) {
                const uint4* q = reinterpret_cast<const uint4*>(p + (size_t)j * pitch);
#pragma unroll
                for (int k = 0; k < S / 4; ++k) {
                    const uint4 v = q[k];
                    resolve_add(s, v.x), resolve_add(s, v.y), resolve_add(s, v.z), resolve_add(s, v.w);
                }
            }
            w[0] = resolve_pack(s, SH);
        } else {
            w[0] = resolve_block<S>(p, pitch);
        }
        const size_t o = (size_t)y * W + x;
#pragma unroll
        for (uint32_t k = 0; k < PX; ++k) {
            if (!RGB8 || out) out[o + k] = w[k];
            if constexpr (RGB8) {       // R first, as pack_rgb8_kernel
                rgb[3 * (o + k) + 0] = (uint8_t)(w[k] >> 16);
                rgb[3 * (o + k) + 1] = (uint8_t)(w[k] >> 8);
                rgb[3 * (o + k) + 2] = (uint8_t)w[k];
            }
        }
    }
}

template <int S, bool VEC>
hipError_t launch_s(const uint32_t* fine, uint32_t W, uint32_t rows, uint32_t* out, uint8_t* rgb, hipStream_t stream) {
    const uint32_t items = (VEC && S == 2) ? W / 2u : W;
    const dim3 grid((items + 255u) / 256u, rows < 65535u ? rows : 65535u), block(256);
    if (rgb)
        hipLaunchKernelGGL((resolve_kernel<S, true, VEC>), grid, block, 0, stream, fine, W, rows, out, rgb);
    else
        hipLaunchKernelGGL((resolve_kernel<S, false, VEC>), grid, block, 0, stream, fine, W, rows, out, rgb);
    return hipGetLastError();
}

}  // namespace

bool resolve_vector_path(const void* fine, uint32_t W, uint32_t S) {
    if (((uintptr_t)fine & 15u) != 0u) return false;
    return S == 4u || S == 8u || (S == 2u && (W & 1u) == 0u);
}

hipError_t launch_resolve(const uint32_t* fine, uint32_t W, uint32_t rows, uint32_t S, uint32_t* out, uint8_t* rgb,
                          hipStream_t stream) {
    if (W == 0 || rows == 0) return hipSuccess;
    const bool vec = resolve_vector_path(fine, W, S);
    switch (S) {
    case 1: return launch_s<1, false>(fine, W, rows, out, rgb, stream);
    case 2: return vec ? launch_s<2, true>(fine, W, rows, out, rgb, stream) : launch_s<2, false>(fine, W, rows, out, rgb, stream);
    case 4: return vec ? launch_s<4, true>(fine, W, rows, out, rgb, stream) : launch_s<4, false>(fine, W, rows, out, rgb, stream);
    case 8: return vec ? launch_s<8, true>(fine, W, rows, out, rgb, stream) : launch_s<8, false>(fine, W, rows, out, rgb, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace vr
