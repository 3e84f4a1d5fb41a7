// vr_reflect.hip -- mirror reflections (include/vr.h vr_bounce_rays, vr_shade_lights_reflect;
// DESIGN.md 4l): the bounce of a ray at its hit, the compact list of the rays that reflect, and the
// fold of a deeper depth's colours into the shallower one's.  The walks and the lighting of every
// depth are vr_lights.hip's launches, unchanged; this unit only makes their rays and index lists
// and blends their words.  The arithmetic is vr_reflect_math.h's.  A unit of its own, so that every
// other kernel is compiled exactly as before.  No LDS, no walk; one atomic per wave in the
// list append and none anywhere else.
#include "vr_internal.h"

#include "vr_lights_state.h"
#include "vr_reflect_math.h"

namespace vr {
namespace {

constexpr uint32_t kReflectThreads = 256;

// vr_bounce_rays: out[i] = bounce(rays[i], hits[i]), one lane per record.  Of the ray only its
// second 16 bytes (the direction) are read, of the record all four; two 16-byte stores.  Any
// bytes are taken: a record that is no VOXEL hit with a unit axis normal gives six quiet NaNs.
__global__ __launch_bounds__(kReflectThreads) void bounce_rays_kernel(const uint4* __restrict__ rays,
                                                                    const uint4* __restrict__ hits, uint32_t n, float tx,
                                                                    float ty, float tz, float scale_f,
                                                                    uint4* __restrict__ out) {
    const uint32_t i = blockIdx.x * kReflectThreads + threadIdx.x;
    if (i >= n) return;
    const uint4 d = rays[(size_t)i * 2u + 1u];
    const uint4* rec = hits + (size_t)i * 4u;
    const uint4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
    // r0 = {status, color, voxel.x, voxel.y}  r1 = {voxel.z, normal.x, normal.y, normal.z}
    // r2 = {region.x, region.y, region.z, point.x}  r3 = {point.y, point.z, reserved, reserved}
    const int a = bounce_axis(r0.x, (int32_t)r1.y, (int32_t)r1.z, (int32_t)r1.w);
    const int32_t region[3] = {(int32_t)r2.x, (int32_t)r2.y, (int32_t)r2.z};
    const float point[3] = {__uint_as_float(r2.w), __uint_as_float(r3.x), __uint_as_float(r3.y)};
    const uint32_t dir[3] = {d.x, d.y, d.z};
    const float tr[3] = {tx, ty, tz};
    uint32_t w[8];
    bounce_ray(a, region, point, dir, tr, scale_f, w);
    out[(size_t)i * 2u] = uint4{w[0], w[1], w[2], w[3]};
    out[(size_t)i * 2u + 1u] = uint4{w[4], w[5], w[6], w[7]};
}

// One depth's descent of vr_shade_lights_reflect.  Lane i takes ray r = prev ? prev[i] : i of the
// n_prev rays alive at the depth above, reads the hit state lights_primary_kernel left for it
// (vr_lights_state.h) and, where the ray hit a voxel whose stored colour passes the mirror test
// (col & mask) == value, writes its bounce into rays_out[r] -- from the state's point and region
// and the direction of rays_in[r], vr_bounce_rays' arithmetic -- and appends r to `list`.  The
// append takes one atomic per wave: the wave's count goes to *count from its first lane and every
// reflecting lane's place is the wave's base plus the reflecting lanes below it.  No lane leaves
// before the ballot, so the whole wave takes part.  `list` holds n_prev words and receives at most
// as many; the order of its entries is the order in which the waves' atomics land, and no word of
// the result depends on it.
__global__ __launch_bounds__(kReflectThreads) void bounce_compact_kernel(const uint4* __restrict__ state,
                                                                       const uint4* __restrict__ rays_in,
                                                                       const uint32_t* __restrict__ prev, uint32_t n_prev,
                                                                       uint32_t mask, uint32_t value, float tx, float ty,
                                                                       float tz, float scale_f, uint4* __restrict__ rays_out,
                                                                       uint32_t* __restrict__ list,
                                                                       uint32_t* __restrict__ count) {
    const uint32_t i = blockIdx.x * kReflectThreads + threadIdx.x;
    const bool live = i < n_prev;
    uint32_t r = 0;
    bool refl = false;
    if (live) {
        r = prev ? prev[i] : i;
        const uint4 a = state[(size_t)r * 2u];
        refl = (a.y & kStHit) != 0u && (a.x & mask) == value;
        if (refl) {
            const uint4 b = state[(size_t)r * 2u + 1u];
            const uint4 d = rays_in[(size_t)r * 2u + 1u];
            const int32_t region[3] = {(int32_t)b.y, (int32_t)b.z, (int32_t)b.w};
            const float point[3] = {__uint_as_float(a.z), __uint_as_float(a.w), __uint_as_float(b.x)};
            const uint32_t dir[3] = {d.x, d.y, d.z};
            const float tr[3] = {tx, ty, tz};
            uint32_t w[8];
            bounce_ray((int)(a.y & 3u), region, point, dir, tr, scale_f, w);
            rays_out[(size_t)r * 2u] = uint4{w[0], w[1], w[2], w[3]};
            rays_out[(size_t)r * 2u + 1u] = uint4{w[4], w[5], w[6], w[7]};
        }
    }
    const uint64_t votes = __ballot(refl);
    const uint32_t lane = __lane_id();
    uint32_t base = 0;
    if (lane == 0u && votes != 0ull) base = atomicAdd(count, (uint32_t)__popcll(votes));
    base = __shfl(base, 0);
    if (refl) list[base + (uint32_t)__popcll(votes & ((1ull << lane) - 1ull))] = r;
}

// One fold of vr_shade_lights_reflect: for every ray r of `list` (the rays that reflected at the
// shallower depth), shallow[r] = mix_rgb(shallow[r], deep[r], k).  Ray r belongs to one lane and
// launches on one stream are ordered, so the read-modify-write needs no atomics.
__global__ __launch_bounds__(kReflectThreads) void fold_kernel(const uint32_t* __restrict__ list, uint32_t n,
                                                             uint32_t* __restrict__ shallow,
                                                             const uint32_t* __restrict__ deep, uint32_t k) {
    const uint32_t i = blockIdx.x * kReflectThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = list[i];
    shallow[r] = mix_rgb(shallow[r], deep[r], k);
}

dim3 grid_of(uint32_t n) { return dim3((n + kReflectThreads - 1u) / kReflectThreads); }

}  // namespace

hipError_t launch_bounce_rays(const void* rays, const void* hits, uint32_t n, const float translation[3], float scale_f,
                              void* out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(bounce_rays_kernel, grid_of(n), dim3(kReflectThreads), 0, stream, static_cast<const uint4*>(rays),
                       static_cast<const uint4*>(hits), n, translation[0], translation[1], translation[2], scale_f,
                       static_cast<uint4*>(out));
    return hipGetLastError();
}

hipError_t launch_bounce_compact(const void* state, const void* rays_in, const uint32_t* prev, uint32_t n_prev,
                                 uint32_t mask, uint32_t value, const float translation[3], float scale_f, void* rays_out,
                                 uint32_t* list, uint32_t* count, hipStream_t stream) {
    if (n_prev == 0) return hipSuccess;
    hipLaunchKernelGGL(bounce_compact_kernel, grid_of(n_prev), dim3(kReflectThreads), 0, stream,
                       static_cast<const uint4*>(state), static_cast<const uint4*>(rays_in), prev, n_prev, mask, value,
                       translation[0], translation[1], translation[2], scale_f, static_cast<uint4*>(rays_out), list, count);
    return hipGetLastError();
}

hipError_t launch_fold(const uint32_t* list, uint32_t n, uint32_t* shallow, const uint32_t* deep, uint32_t k,
                       hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(fold_kernel, grid_of(n), dim3(kReflectThreads), 0, stream, list, n, shallow, deep, k);
    return hipGetLastError();
}

}  // namespace vr
