// vr_atmos_math.h -- the arithmetic of vr_atmosphere_apply and vr_shade_lights_atmosphere
// (include/vr.h): the sky a ray that misses sees and the linear distance fog over a
// voxel hit.  Plain functions that compile for the device (vr_atmos.hip) and for a host compiler
// with nothing from HIP (tools/atmos_check.cpp checks them on a CPU), with the same results on
// both sides: fp32, one rounding per operation, no contraction, the divisions and square roots
// correctly rounded (the library's build flags on the device, IEEE on a host); what reaches a
// colour word goes through q256 first, so no NaN's bits ever show.  The blend is of integers only.
#pragma once

#include <math.h>
#include <stdint.h>

#include "vr_reflect_math.h"

#if defined(__HIPCC__)
#define VR_ATMOS_HD __host__ __device__ __forceinline__
#else
#define VR_ATMOS_HD inline
#endif

namespace vr {

constexpr uint32_t kAtmosSky = 1u, kAtmosFog = 2u;      // VR_ATMOS_SKY, VR_ATMOS_FOG
constexpr uint32_t kAtmosStatusMiss = 0u;               // VR_HIT_MISS (VOXEL: kBounceStatusVoxel)

// A vr_atmosphere as the kernels take it, made once per call on the host (atmos_params): the four
// colours packed as words, up and the fog's bounds as they came, the span fog_end - fog_start (one
// fp32 subtraction, the same on either side) and the flags.  44 bytes: a kernel argument.
struct AtmosParams {
    uint32_t zenith, horizon, nadir, fog;
    float up[3];
    float fog_start, fog_span;
    uint32_t flags;
};

// One colour byte of a float channel, 1.0 = 255: min(255, f2u(x * 255.0f)), f2u as
// ambient_channel's (vr_lights_math.h) -- NaN and values <= 0 give 0, everything else truncates.
// Host side only: the bytes are made once per call.
inline uint32_t atmos_byte(float x) {
    const float f = x * 255.0f;
    if (!(f == f) || f <= 0.0f) return 0u;
    if (f >= 255.0f) return 255u;
    return (uint32_t)f;
}
inline uint32_t atmos_pack(const float c[3]) { return atmos_byte(c[0]) << 16 | atmos_byte(c[1]) << 8 | atmos_byte(c[2]); }

inline AtmosParams atmos_params(const float zenith[3], const float horizon[3], const float nadir[3], const float up[3],
                                const float fog_color[3], float fog_start, float fog_end, uint32_t flags) {
    AtmosParams p;
    p.zenith = atmos_pack(zenith);
    p.horizon = atmos_pack(horizon);
    p.nadir = atmos_pack(nadir);
    p.fog = atmos_pack(fog_color);
    for (int c = 0; c < 3; ++c) p.up[c] = up[c];
    p.fog_start = fog_start;
    p.fog_span = fog_end - fog_start;
    p.flags = flags;
    return p;
}

// A fraction as 0..256: g = f * 256.0f; 0 if !(g > 0) (NaN too), 256 if g >= 256, else (int)g
// (truncated) -- vr_occlusion's position rule (ao_q).
VR_ATMOS_HD uint32_t q256(float f) {
    const float g = f * 256.0f;
    if (!(g > 0.0f)) return 0u;
    if (g >= 256.0f) return 256u;
    return (uint32_t)(int32_t)g;
}

// Words a and b blended by q in 0..256: each of the bytes R, G and B is
// (A * (256 - q) + B * q + 128) >> 8; bits 24-31 are dropped.  q = 0 gives a and q = 256 gives b.
VR_ATMOS_HD uint32_t lerp256_channel(uint32_t a, uint32_t b, uint32_t q) { return (a * (256u - q) + b * q + 128u) >> 8; }
VR_ATMOS_HD uint32_t lerp256(uint32_t a, uint32_t b, uint32_t q) {
    return lerp256_channel((a >> 16) & 0xFFu, (b >> 16) & 0xFFu, q) << 16 |
           lerp256_channel((a >> 8) & 0xFFu, (b >> 8) & 0xFFu, q) << 8 | lerp256_channel(a & 0xFFu, b & 0xFFu, q);
}

// The sky in direction d (any length): h = (d . up) / |d|, the horizon's colour blended towards
// the zenith's (h >= 0) or the nadir's (h < 0) by |h|.  A NaN h (a zero, infinite or NaN
// direction) gives the horizon's colour: q256 of a NaN is 0.
VR_ATMOS_HD uint32_t atmos_sky(const AtmosParams& p, float dx, float dy, float dz) {
    const float len = sqrtf((dx * dx + dy * dy) + dz * dz);
    const float h = ((dx * p.up[0] + dy * p.up[1]) + dz * p.up[2]) / len;
    return lerp256(p.horizon, h < 0.0f ? p.nadir : p.zenith, q256(fabsf(h)));
}

// Word w of a VOXEL hit under the fog: the hit point back in world space (bounce_origin), its
// distance D from the ray's origin, f = (D - fog_start) / (fog_end - fog_start), and w blended
// towards the fog's colour by q256(f).
VR_ATMOS_HD uint32_t atmos_fog(const AtmosParams& p, uint32_t w, const float origin[3], const int32_t region[3],
                               const float point[3], const float translation[3], float scale_f) {
    const float ex = bounce_origin(translation[0], region[0], point[0], scale_f) - origin[0];
    const float ey = bounce_origin(translation[1], region[1], point[1], scale_f) - origin[1];
    const float ez = bounce_origin(translation[2], region[2], point[2], scale_f) - origin[2];
    const float D = sqrtf((ex * ex + ey * ey) + ez * ez);
    const float f = (D - p.fog_start) / p.fog_span;
    return lerp256(w, p.fog, q256(f));
}

// atmos(w, ray, record) from the record's status, region and point: the sky for a MISS when the
// flags have SKY, the fog for a VOXEL hit when they have FOG, w bit for bit for everything else.
VR_ATMOS_HD uint32_t atmos_word(const AtmosParams& p, uint32_t w, uint32_t status, const float origin[3], const float dir[3],
                                const int32_t region[3], const float point[3], const float translation[3], float scale_f) {
    if (status == kAtmosStatusMiss && (p.flags & kAtmosSky)) return atmos_sky(p, dir[0], dir[1], dir[2]);
    if (status == kBounceStatusVoxel && (p.flags & kAtmosFog)) return atmos_fog(p, w, origin, region, point, translation, scale_f);
    return w;
}

}  // namespace vr
