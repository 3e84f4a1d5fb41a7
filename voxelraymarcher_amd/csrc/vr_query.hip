// vr_query.hip -- the query kernels: vr_pick (the hit behind a pixel), vr_trace (closest hits
// for arbitrary rays; its coherent order is vr_trace.hip) and vr_camera_rays.  They walk with
// the exact Walker of vr_walk.h, compiled here with its no-op counting macros: in the
// counting build libvr_cover.so these kernels count nothing.
#include "vr_walk.h"

namespace vr {
namespace {

// Pick (vr_pick): the primary hit of pixel (px[i], py[i]) as a 64-byte record, one lane per
// query, with the exact walker (the crawl pass's: every walk runs to its end, crawls are
// fast-forwarded, a walk that never finishes is detected) and nothing else -- no lighting,
// no shadow walk, no deferral, no byte count.  The view is one band over the whole frame
// (rank 0 of 1), so pixel_ray maps (x, l) to frame pixel (x, y) as a full-frame render does.
// The hit voxel is the cell of the probe that read the colour (PickCell), through the
// store's key x << 20 | y << 10 | z and back: for a cell inside the region that is the
// cell itself; a probe outside it can only match the stored voxel its wrapped key names.
constexpr uint32_t kPickThreads = 256;
template <int STORE, int ALGO>
__global__ __launch_bounds__(kPickThreads) void pick_kernel(KScene s, KView v, const uint32_t* __restrict__ px,
                                                           const uint32_t* __restrict__ py, uint32_t n,
                                                           uint4* __restrict__ hits) {
    const uint32_t i = blockIdx.x * kPickThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t x = px[i], y = py[i];
    uint4 r0{kPickOutside, 0u, 0u, 0u}, r1{0u, 0u, 0u, 0u}, r2{0u, 0u, 0u, 0u}, r3{0u, 0u, 0u, 0u};
    f3 ro, rd;
    if (x < v.W && y < v.H && pixel_ray<true>(v, x, y, ro, rd)) {
        Walker<STORE, false, true, true> w(s, v);
        Hit h;
        const bool hit = w.template primary<ALGO>(ro, rd, h);
        r0.x = w.aborted ? kPickNever : (hit ? kPickVoxel : kPickMiss);
        if (hit && !w.aborted) {
            const uint32_t key = ((uint32_t)w.pv.x << 20) | ((uint32_t)w.pv.y << 10) | (uint32_t)w.pv.z;
            const f3 nrm = w.normal_of(h.nc);
            r0.y = h.col;
            r0.z = (uint32_t)(h.region.x * kBlock) + (key >> 20);
            r0.w = (uint32_t)(h.region.y * kBlock) + ((key >> 10) & 1023u);
            r1.x = (uint32_t)(h.region.z * kBlock) + (key & 1023u);
            r1.y = (uint32_t)(int32_t)nrm.x;
            r1.z = (uint32_t)(int32_t)nrm.y;
            r1.w = (uint32_t)(int32_t)nrm.z;
            r2 = uint4{(uint32_t)h.region.x, (uint32_t)h.region.y, (uint32_t)h.region.z, __float_as_uint(h.so.x)};
            r3 = uint4{__float_as_uint(h.so.y), __float_as_uint(h.so.z), 0u, 0u};
        }
    }
    uint4* rec = hits + (size_t)i * 4u;        // four 16-byte stores
    rec[0] = r0;
    rec[1] = r1;
    rec[2] = r2;
    rec[3] = r3;
}

// Trace (vr_trace): the primary hit of ray r = idx ? idx[i] : i, written to record r -- the pick's
// walker and the pick's record, with the ray loaded (two 16-byte loads: origin, reserved0,
// direction, reserved1) instead of made from a pixel.  The walk's direction is
// makeUnitVector(direction) (Vector3.cuh:162-165), plain IEEE sqrt and divisions: pixel_ray's
// hoisted-reciprocal division is proved for |d| in [2^-64, 2^20] only, and a caller's direction
// has any magnitude.  idx (the coherent order, vr_trace.hip) is a permutation of 0..n-1, so
// every record is written once whatever the order.  Of the view only translation and scale_f
// are read.  (pick_kernel is left as it was; the record assembly is repeated here.  A shared
// device function for it -- returning the record, filling one by reference, or holding the
// whole walk -- was tried when the kernels moved here: each form changed the register
// allocation of all eight walk kernels, profiles/split/README.md.)
template <int STORE, int ALGO>
__global__ __launch_bounds__(kPickThreads) void trace_kernel(KScene s, KView v, const float4* __restrict__ rays,
                                                            const uint32_t* __restrict__ idx, uint32_t n,
                                                            uint4* __restrict__ hits) {
    const uint32_t i = blockIdx.x * kPickThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = idx ? idx[i] : i;
    const float4 a = rays[(size_t)r * 2u], b = rays[(size_t)r * 2u + 1u];
    uint4 r0{kPickMiss, 0u, 0u, 0u}, r1{0u, 0u, 0u, 0u}, r2{0u, 0u, 0u, 0u}, r3{0u, 0u, 0u, 0u};
    {
        Walker<STORE, false, true, true> w(s, v);
        Hit h;
        const bool hit = w.template primary<ALGO>(f3{a.x, a.y, a.z}, unit(f3{b.x, b.y, b.z}), h);
        r0.x = w.aborted ? kPickNever : (hit ? kPickVoxel : kPickMiss);
        if (hit && !w.aborted) {
            const uint32_t key = ((uint32_t)w.pv.x << 20) | ((uint32_t)w.pv.y << 10) | (uint32_t)w.pv.z;
            const f3 nrm = w.normal_of(h.nc);
            r0.y = h.col;
            r0.z = (uint32_t)(h.region.x * kBlock) + (key >> 20);
            r0.w = (uint32_t)(h.region.y * kBlock) + ((key >> 10) & 1023u);
            r1.x = (uint32_t)(h.region.z * kBlock) + (key & 1023u);
            r1.y = (uint32_t)(int32_t)nrm.x;
            r1.z = (uint32_t)(int32_t)nrm.y;
            r1.w = (uint32_t)(int32_t)nrm.z;
            r2 = uint4{(uint32_t)h.region.x, (uint32_t)h.region.y, (uint32_t)h.region.z, __float_as_uint(h.so.x)};
            r3 = uint4{__float_as_uint(h.so.y), __float_as_uint(h.so.z), 0u, 0u};
        }
    }
    uint4* rec = hits + (size_t)r * 4u;        // four 16-byte stores
    rec[0] = r0;
    rec[1] = r1;
    rec[2] = r2;
    rec[3] = r3;
}

// vr_camera_rays: pixel (px[i], py[i]) of the view's frame (one band, rank 0 of 1, as the pick's)
// as a vr_ray -- origin the image-plane point pixel_ray<true> makes, direction origin - eye, the
// vector pixel_ray normalises (not normalised here: trace_kernel's unit() divides it exactly as
// pixel_ray's correctly rounded division does).  A pixel outside the frame: six quiet NaNs.
__global__ __launch_bounds__(kPickThreads) void camera_rays_kernel(KView v, const uint32_t* __restrict__ px,
                                                                  const uint32_t* __restrict__ py, uint32_t n,
                                                                  uint4* __restrict__ rays) {
    const uint32_t i = blockIdx.x * kPickThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t x = px[i], y = py[i];
    constexpr uint32_t kNaN = 0x7FC00000u;
    uint4 o{kNaN, kNaN, kNaN, 0u}, d{kNaN, kNaN, kNaN, 0u};
    f3 ro, rd;
    if (x < v.W && y < v.H && pixel_ray<true>(v, x, y, ro, rd)) {
        const f3 c = sub(ro, ld3(v.org));
        o = uint4{__float_as_uint(ro.x), __float_as_uint(ro.y), __float_as_uint(ro.z), 0u};
        d = uint4{__float_as_uint(c.x), __float_as_uint(c.y), __float_as_uint(c.z), 0u};
    }
    rays[(size_t)i * 2u] = o;
    rays[(size_t)i * 2u + 1u] = d;
}

}  // namespace

hipError_t launch_pick(int store, int algo, const KScene& s, const KView& v, const uint32_t* px, const uint32_t* py,
                       uint32_t n, void* hits, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const dim3 grid((n + kPickThreads - 1u) / kPickThreads), block(kPickThreads);
    uint4* out = static_cast<uint4*>(hits);
    for_store_algo(store, algo, [&](auto st, auto al) {
        hipLaunchKernelGGL((pick_kernel<decltype(st)::value, decltype(al)::value>), grid, block, 0, stream, s, v, px, py,
                           n, out);
    });
    return hipGetLastError();
}

hipError_t launch_trace(int store, int algo, const KScene& s, const KView& v, const void* rays, const uint32_t* idx,
                        uint32_t n, void* hits, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const dim3 grid((n + kPickThreads - 1u) / kPickThreads), block(kPickThreads);
    const float4* in = static_cast<const float4*>(rays);
    uint4* out = static_cast<uint4*>(hits);
    for_store_algo(store, algo, [&](auto st, auto al) {
        hipLaunchKernelGGL((trace_kernel<decltype(st)::value, decltype(al)::value>), grid, block, 0, stream, s, v, in, idx,
                           n, out);
    });
    return hipGetLastError();
}

hipError_t launch_camera_rays(const KView& v, const uint32_t* px, const uint32_t* py, uint32_t n, void* rays,
                              hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(camera_rays_kernel, dim3((n + kPickThreads - 1u) / kPickThreads), dim3(kPickThreads), 0, stream, v,
                       px, py, n, static_cast<uint4*>(rays));
    return hipGetLastError();
}

}  // namespace vr
