// vr_reflect_math.h -- the arithmetic of vr_bounce_rays and vr_shade_lights_reflect (include/vr.h,
// DESIGN.md 4l): the mirror bounce of a ray at a hit and the blend of two colour words.  Plain
// functions that compile for the device (vr_reflect.hip) and for a host compiler with nothing from
// HIP (tools/reflect_check.cpp checks them on a CPU), with the same results on both sides: the
// bounce is five fp32 operations per component, no contraction, the division correctly rounded,
// and one flipped sign bit; the blend is of integers only.
#pragma once

#include <stdint.h>

#include "vr_occlusion_math.h"

#if defined(__HIPCC__)
#define VR_REFLECT_HD __host__ __device__ __forceinline__
#else
#define VR_REFLECT_HD inline
#endif

namespace vr {

constexpr uint32_t kQuietNaN = 0x7FC00000u;          // what vr_camera_rays writes for a pixel outside the frame
constexpr uint32_t kBounceStatusVoxel = 1u;          // VR_HIT_VOXEL

VR_REFLECT_HD uint32_t reflect_bits(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, sizeof u);
    return u;
}

// The axis a bounce reflects about: the axis of the record's normal when the record is a VOXEL hit
// whose normal has exactly one component +1 or -1 and the others 0 (vr_occlusion's condition,
// ao_axis); -1 for every other record: no bounce.
VR_REFLECT_HD int bounce_axis(uint32_t status, int32_t nx, int32_t ny, int32_t nz) {
    return status == kBounceStatusVoxel ? ao_axis(nx, ny, nz) : -1;
}

// One component of the bounce ray's origin, the hit's point back in world space:
// translation + ((float)region * 64.0f + point) / scale_f -- int-to-float, multiply, add, divide,
// add, each rounded to fp32 on its own, in that order.  scale_f is (float)scale.
VR_REFLECT_HD float bounce_origin(float translation, int32_t region, float point, float scale_f) {
    const float r = (float)region;
    const float m = r * 64.0f;
    const float s = m + point;
    const float q = s / scale_f;
    return translation + q;
}

// The bits of one component of the bounce ray's direction: those of the incoming direction, with
// the sign bit flipped on the normal's axis (a zero, an infinity and a NaN have their sign flipped
// too).  Nothing is normalised: the magnitude survives every depth.
VR_REFLECT_HD uint32_t bounce_direction(uint32_t dir_bits, bool on_axis) { return on_axis ? dir_bits ^ 0x80000000u : dir_bits; }

// The bounce of the ray whose direction bits are dir[3] at a hit with axis a (bounce_axis), region
// and point: out[0..7] are the eight words of a vr_ray (reserved0 and reserved1 0).  With a < 0
// all six floats are the quiet NaN.
VR_REFLECT_HD void bounce_ray(int a, const int32_t region[3], const float point[3], const uint32_t dir[3],
                              const float translation[3], float scale_f, uint32_t out[8]) {
    out[3] = 0u;
    out[7] = 0u;
    for (int c = 0; c < 3; ++c) {
        out[c] = a < 0 ? kQuietNaN : reflect_bits(bounce_origin(translation[c], region[c], point[c], scale_f));
        out[4 + c] = a < 0 ? kQuietNaN : bounce_direction(dir[c], c == a);
    }
}

// Words a and b blended by k in 0..255: each of the bytes R, G and B is
// (A * (255 - k) + B * k + 127) / 255, an integer division; bits 24-31 are dropped.  k = 0 gives a
// and k = 255 gives b (for words whose bits 24-31 are clear).
VR_REFLECT_HD uint32_t mix_channel(uint32_t a, uint32_t b, uint32_t k) { return (a * (255u - k) + b * k + 127u) / 255u; }
VR_REFLECT_HD uint32_t mix_rgb(uint32_t a, uint32_t b, uint32_t k) {
    return mix_channel((a >> 16) & 0xFFu, (b >> 16) & 0xFFu, k) << 16 | mix_channel((a >> 8) & 0xFFu, (b >> 8) & 0xFFu, k) << 8 |
           mix_channel(a & 0xFFu, b & 0xFFu, k);
}

}  // namespace vr
