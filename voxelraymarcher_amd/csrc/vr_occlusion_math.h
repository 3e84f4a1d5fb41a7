// vr_occlusion_math.h -- the arithmetic of vr_occlusion and vr_shade_lights_ao (include/vr.h,
// DESIGN.md 4k): the corner levels of a face's eight neighbours, the position on the face in
// 1/256ths, the bilinear sum in integers, the factor a strength makes of it and the scaling of a
// colour word.  All integer after one fp32 subtraction.  Plain functions that compile for the
// device (vr_occlusion.hip) and for a host compiler with nothing from HIP (tools/ao_check.cpp
// checks them on a CPU), with the same results on both sides.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define VR_AO_HD __host__ __device__ __forceinline__
#else
#define VR_AO_HD inline
#endif

namespace vr {

constexpr uint32_t kAoOpen = 255u;          // VR_AO_OPEN

// The eight neighbours of the plane cell p in the face's plane, as (du, dw) along the tangent
// axes: bit j of an occupancy pattern is o(ao_du(j), ao_dw(j)) -- the 3 x 3 cells row by row,
// du fastest, the centre left out: (-1,-1) (0,-1) (1,-1) (-1,0) (1,0) (-1,1) (0,1) (1,1).
VR_AO_HD int ao_du(int j) { return (j < 4 ? j : j + 1) % 3 - 1; }
VR_AO_HD int ao_dw(int j) { return (j < 4 ? j : j + 1) / 3 - 1; }

// The axis a (0, 1, 2) of a normal with exactly one component +1 or -1 and the others 0; -1 for
// every other normal.
VR_AO_HD int ao_axis(int32_t nx, int32_t ny, int32_t nz) {
    const bool ux = nx == 1 || nx == -1, uy = ny == 1 || ny == -1, uz = nz == 1 || nz == -1;
    if (ux && ny == 0 && nz == 0) return 0;
    if (uy && nx == 0 && nz == 0) return 1;
    if (uz && nx == 0 && ny == 0) return 2;
    return -1;
}

// The tangent axes (u, w) of axis a: (1, 2), (2, 0), (0, 1).
VR_AO_HD int ao_axis_u(int a) { return a == 0 ? 1 : (a == 1 ? 2 : 0); }
VR_AO_HD int ao_axis_w(int a) { return a == 0 ? 2 : (a == 1 ? 0 : 1); }

// The level of a corner from its two side cells and its corner cell (each 0 or 1): 0 when both
// sides are stored, else 3 - (s1 + s2 + c).
VR_AO_HD uint32_t ao_corner(uint32_t s1, uint32_t s2, uint32_t c) { return (s1 & s2) ? 0u : 3u - (s1 + s2 + c); }

// The four corner levels of an occupancy pattern, L(-1,-1) | L(+1,-1) << 2 | L(-1,+1) << 4 | L(+1,+1) << 6.
VR_AO_HD uint32_t ao_levels(uint32_t occ) {
    const uint32_t mm = occ & 1u, zm = (occ >> 1) & 1u, pm = (occ >> 2) & 1u, mz = (occ >> 3) & 1u, pz = (occ >> 4) & 1u,
                   mp = (occ >> 5) & 1u, zp = (occ >> 6) & 1u, pp = (occ >> 7) & 1u;
    return ao_corner(mz, zm, mm) | ao_corner(pz, zm, pm) << 2 | ao_corner(mz, zp, mp) << 4 | ao_corner(pz, zp, pp) << 6;
}

// The position on the face along one tangent axis, in 0..256: point - (float)(int32)(voxel -
// 64 * region) is one fp32 subtraction (the integer part wraps), times 256.0f (exact), clamped
// (NaN and everything not above 0 give 0) and truncated.
VR_AO_HD uint32_t ao_q(float point, int32_t voxel, int32_t region) {
    const int32_t local = (int32_t)((uint32_t)voxel - 64u * (uint32_t)region);
    const float f = point - (float)local;
    const float g = f * 256.0f;
    if (!(g > 0.0f)) return 0u;
    if (g >= 256.0f) return 256u;
    return (uint32_t)(int32_t)g;
}

// The bilinear sum of the four levels at (qu, qw), each in 0..256: at most 3 * 65536.
VR_AO_HD uint32_t ao_acc(uint32_t levels, uint32_t qu, uint32_t qw) {
    const uint32_t l00 = levels & 3u, l10 = (levels >> 2) & 3u, l01 = (levels >> 4) & 3u, l11 = (levels >> 6) & 3u;
    return (256u - qu) * (256u - qw) * l00 + qu * (256u - qw) * l10 + (256u - qu) * qw * l01 + qu * qw * l11;
}

// acc of 0..3 * 65536 as 0..255, rounded to nearest.
VR_AO_HD uint32_t ao_round(uint32_t acc) { return (acc * 255u + 98304u) / 196608u; }

// ao of an occupancy pattern and a position on the face.
VR_AO_HD uint32_t ao_value(uint32_t occ, uint32_t qu, uint32_t qw) { return ao_round(ao_acc(ao_levels(occ), qu, qw)); }

// The factor m a strength in 0..255 makes of ao: 255 at strength 0, ao at strength 255.
VR_AO_HD uint32_t ao_factor(uint32_t ao, uint32_t strength) { return 255u - ((255u - ao) * strength + 127u) / 255u; }

// Each of the bytes R, G and B of `word` replaced by (b * m + 127) / 255, m in 0..255; bits 24-31
// are dropped.
VR_AO_HD uint32_t scale_rgb(uint32_t word, uint32_t m) {
    const uint32_t r = (((word >> 16) & 0xFFu) * m + 127u) / 255u, g = (((word >> 8) & 0xFFu) * m + 127u) / 255u,
                   b = ((word & 0xFFu) * m + 127u) / 255u;
    return r << 16 | g << 8 | b;
}

}  // namespace vr
