// vr_shade.hip -- the kernel of vr_shade (include/vr.h): the lit, shadowed colour a render writes
// for a pixel, for a ray that is no pixel of a camera -- and, on request, the hit record
// vr_trace writes for it, from the same walk.  A unit of its own, so that the pick and trace
// kernels of vr_query.hip are compiled exactly as before; the walker is vr_walk.h's with its
// no-op counting macros (in the counting build libvr_cover.so this kernel counts nothing).
#include "vr_walk.h"

namespace vr {
namespace {

// Shade (vr_shade): ray r = idx ? idx[i] : i, loaded as trace_kernel loads it (two 16-byte loads;
// idx is the coherent order of vr_trace.hip, a permutation of 0..n-1), walked by the exact walker
// (the crawl pass's: every walk runs to its end, crawls are fast-forwarded, a walk that never
// finishes is detected), then lit and shadowed as the render's pixel is: light_and_shadow
// (vr_walk.h) at the primary hit, the shadow walk from the hit's point in the hit's region.
// colors[r] is that word; a miss, or a primary or shadow walk that never ends, is 0 (as shade()
// of vr_march.hip writes it).  Nothing is deferred and nothing of the view below `out` is read:
// no deferral list, no pcost, no byte count, no LDS cluster-bit slot (Walker::lbm stays null).
// HITS: the walker is the pick's (PickCell) and record r is written too -- trace_kernel's record
// and its four 16-byte stores, made before the shadow walk starts, so that the record's sixteen
// words are not live through it and a shadow walk that never ends leaves the primary's VOXEL
// record beside colour 0.  Without HITS the walker is the crawl pass's own and `hits` is not read.
// (The record assembly is repeated from trace_kernel, as trace_kernel repeats pick_kernel's:
// see the comment there.)
// 256 threads, as the pick and the trace: no instantiation spills to scratch
// (profiles/shade/README.md has the figures beside crawl_kernel's).
constexpr uint32_t kShadeThreads = 256;
template <int STORE, int ALGO, bool HITS>
__global__ __launch_bounds__(kShadeThreads) void shade_rays_kernel(KScene s, KView v, const float4* __restrict__ rays,
                                                                  const uint32_t* __restrict__ idx, uint32_t n,
                                                                  uint32_t* __restrict__ colors,
                                                                  uint4* __restrict__ hits) {
    const uint32_t i = blockIdx.x * kShadeThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = idx ? idx[i] : i;
    const float4 a = rays[(size_t)r * 2u], b = rays[(size_t)r * 2u + 1u];
    uint32_t col = 0;
    {
        Walker<STORE, false, true, HITS> w(s, v);
        Hit h;
        const bool hit = w.template primary<ALGO>(f3{a.x, a.y, a.z}, unit(f3{b.x, b.y, b.z}), h) && !w.aborted;
        if constexpr (HITS) {
            uint4 r0{w.aborted ? kPickNever : (hit ? kPickVoxel : kPickMiss), 0u, 0u, 0u};
            uint4 r1{0u, 0u, 0u, 0u}, r2{0u, 0u, 0u, 0u}, r3{0u, 0u, 0u, 0u};
            if (hit) {
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
            uint4* rec = hits + (size_t)r * 4u;        // four 16-byte stores
            rec[0] = r0;
            rec[1] = r1;
            rec[2] = r2;
            rec[3] = r3;
        }
        if (hit) {
            col = light_and_shadow<ALGO>(w, v, h);
            if (w.aborted) col = 0;                    // the shadow walk never ends
        }
    }
    colors[r] = col;
}

}  // namespace

hipError_t launch_shade(int store, int algo, const KScene& s, const KView& v, const void* rays, const uint32_t* idx,
                        uint32_t n, uint32_t* colors, void* hits, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const dim3 grid((n + kShadeThreads - 1u) / kShadeThreads), block(kShadeThreads);
    const float4* in = static_cast<const float4*>(rays);
    uint4* out = static_cast<uint4*>(hits);
    for_store_algo(store, algo, [&](auto st, auto al) {
        constexpr int ST = decltype(st)::value, AL = decltype(al)::value;
        if (out) hipLaunchKernelGGL((shade_rays_kernel<ST, AL, true>), grid, block, 0, stream, s, v, in, idx, n, colors, out);
        else hipLaunchKernelGGL((shade_rays_kernel<ST, AL, false>), grid, block, 0, stream, s, v, in, idx, n, colors, out);
    });
    return hipGetLastError();
}

}  // namespace vr
