// vr_resolve_math.h -- the per-pixel arithmetic of vr_resolve (include/vr.h): the box filter of an
// S x S block of packed 0x00RRGGBB words, per channel (sum + N/2) >> log2(N) with N = S * S.
// Plain functions that compile for the device (vr_resolve.hip) and for a host compiler with nothing
// from HIP (tools/resolve_check.cpp checks them on a CPU), with the same results on both sides:
// the arithmetic is of unsigned integers only.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VR_RESOLVE_HD __host__ __device__ __forceinline__
#else
#define VR_RESOLVE_HD inline
#endif

namespace vr {

// log2 of the samples per pixel N = S * S, S in {1, 2, 4, 8}.
template <int S>
struct ResolveShift {
    static_assert(S == 1 || S == 2 || S == 4 || S == 8, "samples per axis");
    static constexpr uint32_t value = S == 1 ? 0u : S == 2 ? 2u : S == 4 ? 4u : 6u;
};

// The channel sums of the words folded in so far.  Red and blue share a word: a channel's sum is
// at most 255 * 64 = 16320 < 2^16, so blue (bits 0-15) never carries into red (bits 16-31).  Bits
// 24-31 of a fine word are dropped by the masks.
struct ResolveSum {
    uint32_t rb, g;
};

VR_RESOLVE_HD void resolve_add(ResolveSum& a, uint32_t w) {
    a.rb += w & 0x00FF00FFu;
    a.g += (w >> 8) & 0xFFu;
}

// One channel's mean of n = 1 << shift values whose sum is `sum`, rounded half up.
VR_RESOLVE_HD uint32_t resolve_mean(uint32_t sum, uint32_t shift) {
    return (sum + ((1u << shift) >> 1)) >> shift;
}

// The resolved word of a pixel from its channel sums: R << 16 | G << 8 | B.
VR_RESOLVE_HD uint32_t resolve_pack(const ResolveSum& a, uint32_t shift) {
    return resolve_mean(a.rb >> 16, shift) << 16 | resolve_mean(a.g, shift) << 8 | resolve_mean(a.rb & 0xFFFFu, shift);
}

// The resolved word of the S x S block whose top left word is p[0], in a fine frame of `pitch`
// words per row: S * S loads of one word each.
template <int S>
VR_RESOLVE_HD uint32_t resolve_block(const uint32_t* p, size_t pitch) {
    ResolveSum a = {0u, 0u};
    for (int j = 0; j < S; ++j)
        for (int i = 0; i < S; ++i) resolve_add(a, p[(size_t)j * pitch + (size_t)i]);
    return resolve_pack(a, ResolveShift<S>::value);
}

}  // namespace vr
