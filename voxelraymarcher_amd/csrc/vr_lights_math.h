// vr_lights_math.h -- the two pieces of arithmetic vr_shade_lights (include/vr.h) adds to the
// walks: the byte-wise saturating sum of its terms and the ambient term.  Plain functions that
// compile for the device (vr_lights.hip, after vr_device.h) and for a host compiler with nothing
// from HIP (tools/lights_check.cpp checks them on a CPU), with the same results on both sides.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define VR_LIGHTS_HD __host__ __device__ __forceinline__
#else
#define VR_LIGHTS_HD inline
#endif

namespace vr {

// The channels of a and b summed byte-wise, each sum clamped at 255:
//   min(255, R(a) + R(b)) << 16 | min(255, G(a) + G(b)) << 8 | min(255, B(a) + B(b)),
// R(w) = (w >> 16) & 0xFF, G(w) = (w >> 8) & 0xFF, B(w) = w & 0xFF.  Bits 24-31 of either word
// are dropped (a term has them only where a light's colour or an un-normalised direction pushed
// a channel past 255 and the reference's packing bled).  No carry crosses a channel.  The sums
// are of non-negative integers, so folding terms in one at a time gives min(255, sum of all) per
// channel whatever their order.
VR_LIGHTS_HD uint32_t sat_add_rgb(uint32_t a, uint32_t b) {
    // red and blue in one word (bits 16-24 and 0-8 hold their 9-bit sums), green in another
    const uint32_t rb = (a & 0x00FF00FFu) + (b & 0x00FF00FFu);
    const uint32_t g = (a & 0x0000FF00u) + (b & 0x0000FF00u);
    const uint32_t r = rb >> 16, bl = rb & 0x1FFu, gr = g >> 8;
    return (r > 255u ? 255u : r) << 16 | (gr > 255u ? 255u : gr) << 8 | (bl > 255u ? 255u : bl);
}

// One channel of the ambient term: f2u((c / 255.0f * a) * 255.0f) for a stored channel c in
// [0, 255] -- the directional formula of Ctx::lighting (vr_device.h) with diff = 1.0f (1.0f * a is
// a, NaN included) and the light's colour replaced by a.  fp32, no contraction; the division is
// correctly rounded on both sides (div255 on the device) and the conversion is v_cvt_u32_f32's:
// NaN and negatives give 0, values of 2^32 and more 0xFFFFFFFF, everything else truncates.
VR_LIGHTS_HD uint32_t ambient_channel(uint32_t c, float a) {
#if defined(__HIP_DEVICE_COMPILE__)
    return f2u((div255(c) * a) * 255.0f);
#else
    const float t = (float)c / 255.0f;
    const float p = t * a;
    const float f = p * 255.0f;
    if (!(f == f) || f <= 0.0f) return 0u;
    if (f >= 0x1p+32f) return 0xFFFFFFFFu;
    return (uint32_t)f;
#endif
}

// The ambient term of a voxel whose stored colour is col (< 2^24): the three channels packed as
// the reference packs a lit colour, R << 16 | G << 8 | B (a channel past 255 bleeds, as there).
VR_LIGHTS_HD uint32_t ambient_term(uint32_t col, float amb_r, float amb_g, float amb_b) {
    const uint32_t R = ambient_channel(col >> 16, amb_r), G = ambient_channel((col >> 8) & 0xFFu, amb_g),
                   B = ambient_channel(col & 0xFFu, amb_b);
    return (R << 16) | (G << 8) | B;
}
VR_LIGHTS_HD uint32_t ambient_term(uint32_t col, const float amb[3]) { return ambient_term(col, amb[0], amb[1], amb[2]); }

}  // namespace vr
