// vr_atmos.hip -- sky and distance fog (include/vr.h vr_atmosphere_apply,
// vr_shade_lights_atmosphere): one elementwise pass that replaces a colour word by
// atmos(word, ray, hit) -- the sky's colour for a ray that missed, the word blended towards the
// fog's colour by the hit's distance for a voxel hit.  The arithmetic is vr_atmos_math.h's.  A
// unit of its own, so that every other kernel is compiled exactly as before.  No LDS, no atomics,
// no walk: every lane owns one ray and one colour word.
#include "vr_internal.h"

#include "vr_atmos_math.h"
#include "vr_lights_state.h"

namespace vr {
namespace {

constexpr uint32_t kAtmosThreads = 256;

// vr_shade_lights_atmosphere's pass for one depth, after that depth's last colour pass on the
// same stream.  Lane i takes ray r = list ? list[i] : i, reads the first 16-byte word of the hit
// state lights_primary_kernel left for it (vr_lights_state.h) and
//   a hit (kStHit), FOG set     reads the state's second word and the ray's origin word, and
//                               blends colors[r] towards the fog's colour;
//   a miss (neither kStHit nor kStNever), SKY set
//                               reads the ray's direction word and writes the sky to colors[r];
//   everything else             touches nothing more (a kStNever ray keeps its word).
// Ray r belongs to one lane and launches on one stream are ordered: the read-modify-write needs
// no atomics.  At depth j >= 1 the state of a ray outside the list is stale: the list is the bound.
__global__ __launch_bounds__(kAtmosThreads) void atmos_state_kernel(const uint4* __restrict__ state,
                                                                  const uint4* __restrict__ rays,
                                                                  const uint32_t* __restrict__ list, uint32_t n,
                                                                  AtmosParams p, float tx, float ty, float tz, float scale_f,
                                                                  uint32_t* __restrict__ colors) {
    const uint32_t i = blockIdx.x * kAtmosThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = list ? list[i] : i;
    const uint4 a = state[(size_t)r * 2u];
    if (a.y & kStHit) {
        if (!(p.flags & kAtmosFog)) return;
        const uint4 b = state[(size_t)r * 2u + 1u];
        const uint4 o = rays[(size_t)r * 2u];
        const float origin[3] = {__uint_as_float(o.x), __uint_as_float(o.y), __uint_as_float(o.z)};
        const int32_t region[3] = {(int32_t)b.y, (int32_t)b.z, (int32_t)b.w};
        const float point[3] = {__uint_as_float(a.z), __uint_as_float(a.w), __uint_as_float(b.x)};
        const float tr[3] = {tx, ty, tz};
        colors[r] = atmos_fog(p, colors[r], origin, region, point, tr, scale_f);
    } else if (!(a.y & kStNever)) {
        if (!(p.flags & kAtmosSky)) return;
        const uint4 d = rays[(size_t)r * 2u + 1u];
        colors[r] = atmos_sky(p, __uint_as_float(d.x), __uint_as_float(d.y), __uint_as_float(d.z));
    }
}

// vr_atmosphere_apply: out[i] = atmos(in[i], rays[i], hits[i]), one lane per record.  The record's
// first 16-byte word gives the status; a VOXEL record under FOG has its last two words and the
// ray's origin word read, a MISS under SKY the ray's direction word.  Any bytes are taken.  out may
// be in: lane i reads in[i] before it writes out[i] and no other lane touches either.
__global__ __launch_bounds__(kAtmosThreads) void atmos_records_kernel(const uint4* __restrict__ rays,
                                                                    const uint4* __restrict__ hits, const uint32_t* in,
                                                                    uint32_t n, AtmosParams p, float tx, float ty, float tz,
                                                                    float scale_f, uint32_t* out) {
    const uint32_t i = blockIdx.x * kAtmosThreads + threadIdx.x;
    if (i >= n) return;
    const uint4* rec = hits + (size_t)i * 4u;
    const uint32_t status = rec[0].x;
    uint32_t w = in[i];
    // r2 = {region.x, region.y, region.z, point.x}  r3 = {point.y, point.z, reserved, reserved}
    if (status == kBounceStatusVoxel && (p.flags & kAtmosFog)) {
        const uint4 r2 = rec[2], r3 = rec[3];
        const uint4 o = rays[(size_t)i * 2u];
        const float origin[3] = {__uint_as_float(o.x), __uint_as_float(o.y), __uint_as_float(o.z)};
        const int32_t region[3] = {(int32_t)r2.x, (int32_t)r2.y, (int32_t)r2.z};
        const float point[3] = {__uint_as_float(r2.w), __uint_as_float(r3.x), __uint_as_float(r3.y)};
        const float tr[3] = {tx, ty, tz};
        w = atmos_fog(p, w, origin, region, point, tr, scale_f);
    } else if (status == kAtmosStatusMiss && (p.flags & kAtmosSky)) {
        const uint4 d = rays[(size_t)i * 2u + 1u];
        w = atmos_sky(p, __uint_as_float(d.x), __uint_as_float(d.y), __uint_as_float(d.z));
    }
    out[i] = w;
}

dim3 grid_of(uint32_t n) { return dim3((n + kAtmosThreads - 1u) / kAtmosThreads); }

}  // namespace

hipError_t launch_atmos_state(const void* state, const void* rays, const uint32_t* list, uint32_t n, const AtmosParams& p,
                              const float translation[3], float scale_f, uint32_t* colors, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(atmos_state_kernel, grid_of(n), dim3(kAtmosThreads), 0, stream, static_cast<const uint4*>(state),
                       static_cast<const uint4*>(rays), list, n, p, translation[0], translation[1], translation[2], scale_f,
                       colors);
    return hipGetLastError();
}

hipError_t launch_atmos_records(const void* rays, const void* hits, const uint32_t* in, uint32_t n, const AtmosParams& p,
                                const float translation[3], float scale_f, uint32_t* out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(atmos_records_kernel, grid_of(n), dim3(kAtmosThreads), 0, stream, static_cast<const uint4*>(rays),
                       static_cast<const uint4*>(hits), in, n, p, translation[0], translation[1], translation[2], scale_f, out);
    return hipGetLastError();
}

}  // namespace vr
