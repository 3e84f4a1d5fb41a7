// vr_lights.hip -- the kernels of vr_shade_lights (include/vr.h): one primary walk per ray, then
// one lighting-and-shadow pass per light over the hits it left, the terms summed byte-wise with a
// clamp at 255 per channel (vr_lights_math.h).  A unit of its own, so that every other kernel is
// compiled exactly as before; the walker is vr_walk.h's with its no-op counting macros (in the
// counting build libvr_cover.so these kernels count nothing).  No field is added to KView: what
// the kernels need beside a view travels as separate arguments.
#include "vr_walk.h"

#include "vr_lights_math.h"
#include "vr_lights_state.h"

namespace vr {
namespace {

// (The per-ray hit state between the two kernels, 32 bytes as two 16-byte words, and its flags
// kStLongest, kStHit and kStNever: vr_lights_state.h.)

// Pass 1: ray r = idx ? idx[i] : i, loaded and walked as shade_rays_kernel (vr_shade.hip) does it
// -- the exact walker, every walk run to its end, a walk that never finishes detected.  Writes
// the state above, colors[r] = the ambient term of the hit's stored colour with bits 24-31
// dropped (has_amb; 0 otherwise, and 0 for a miss or a walk that never ends), and with HITS the
// record shade_rays_kernel writes, by the same assembly and four 16-byte stores (the walker is
// then the pick's).  The state goes out before the record, so that the record's sixteen words are
// assembled with the state's registers free.  Of the view only translation and scale_f are read.
// 256 threads, as the shade: no instantiation spills a register to scratch or touches scratch
// (profiles/lights/README.md has the figures beside shade_rays_kernel's).
constexpr uint32_t kLightsThreads = 256;
template <int STORE, int ALGO, bool HITS>
__global__ __launch_bounds__(kLightsThreads) void lights_primary_kernel(KScene s, KView v, const float4* __restrict__ rays,
                                                                       const uint32_t* __restrict__ idx, uint32_t n,
                                                                       uint32_t has_amb, float amb_r, float amb_g, float amb_b,
                                                                       uint4* __restrict__ state,
                                                                       uint32_t* __restrict__ colors,
                                                                       uint4* __restrict__ hits) {
    const uint32_t i = blockIdx.x * kLightsThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = idx ? idx[i] : i;
    const float4 a = rays[(size_t)r * 2u], b = rays[(size_t)r * 2u + 1u];
    Walker<STORE, false, true, HITS> w(s, v);
    Hit h;
    const bool hit = w.template primary<ALGO>(f3{a.x, a.y, a.z}, unit(f3{b.x, b.y, b.z}), h) && !w.aborted;
    uint4 s0{0u, w.aborted ? kStNever : 0u, 0u, 0u}, s1{0u, 0u, 0u, 0u};
    uint32_t col = 0;
    if (hit) {
        s0 = uint4{h.col, h.nc | (h.longest ? kStLongest : 0u) | kStHit, __float_as_uint(h.so.x), __float_as_uint(h.so.y)};
        s1 = uint4{__float_as_uint(h.so.z), (uint32_t)h.region.x, (uint32_t)h.region.y, (uint32_t)h.region.z};
        if (has_amb) col = sat_add_rgb(0u, ambient_term(h.col, amb_r, amb_g, amb_b));
    }
    uint4* st = state + (size_t)r * 2u;                // two 16-byte stores
    st[0] = s0;
    st[1] = s1;
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
    colors[r] = col;
}

// Pass 2, once per light on the same stream: the light travels in a KView made by view_lighting
// (L, Lr, L_fast, Lw, L_order and the rest stay kernel arguments in SGPRs, the shadow walk's sign
// arms scalar branches).  A lane reloads its ray's state, leaves if the ray has no hit, and
// otherwise runs light_and_shadow with a fresh walker: the term vr_shade writes for the ray under
// this light (0 for a shadow walk that never ends), folded into colors[r].  The fresh walker
// carries nothing over from the primary walk -- the only thing that differs from the one walker of
// shade_rays_kernel is the 2^30 hang-guard count (Ctx::iters), which starts at 0 for the shadow
// walk instead of at the primary walk's length; no finite walk approaches it, and a walk that
// never ends is found by the exact walker's cycle test, not by the count.
// Launches on one stream are ordered and ray r belongs to one lane, so the read-modify-write of
// colors[r] needs no atomics.
template <int STORE, int ALGO>
__global__ __launch_bounds__(kLightsThreads) void light_term_kernel(KScene s, KView v, const uint32_t* __restrict__ idx,
                                                                   uint32_t n, const uint4* __restrict__ state,
                                                                   uint32_t* __restrict__ colors) {
    const uint32_t i = blockIdx.x * kLightsThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = idx ? idx[i] : i;
    const uint4* st = state + (size_t)r * 2u;
    const uint4 a = st[0];
    if (!(a.y & kStHit)) return;
    const uint4 b = st[1];
    Hit h;
    h.col = a.x;
    h.nc = a.y & ~kStFlags;
    h.so = f3{__uint_as_float(a.z), __uint_as_float(a.w), __uint_as_float(b.x)};
    h.region = i3{(int32_t)b.y, (int32_t)b.z, (int32_t)b.w};
    h.longest = (a.y & kStLongest) != 0u;
    Walker<STORE, false, true, false> w(s, v);
    uint32_t term = light_and_shadow<ALGO>(w, v, h);
    if (w.aborted) term = 0;                           // the shadow walk never ends
    colors[r] = sat_add_rgb(colors[r], term);
}

}  // namespace

hipError_t launch_lights_primary(int store, int algo, const KScene& s, const KView& v, const void* rays,
                                 const uint32_t* idx, uint32_t n, const float* ambient, void* state, uint32_t* colors,
                                 void* hits, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const dim3 grid((n + kLightsThreads - 1u) / kLightsThreads), block(kLightsThreads);
    const float4* in = static_cast<const float4*>(rays);
    uint4* st = static_cast<uint4*>(state);
    uint4* out = static_cast<uint4*>(hits);
    const uint32_t has_amb = ambient ? 1u : 0u;
    const float ar = ambient ? ambient[0] : 0.0f, ag = ambient ? ambient[1] : 0.0f, ab = ambient ? ambient[2] : 0.0f;
    for_store_algo(store, algo, [&](auto sto, auto al) {
        constexpr int ST = decltype(sto)::value, AL = decltype(al)::value;
        if (out)
            hipLaunchKernelGGL((lights_primary_kernel<ST, AL, true>), grid, block, 0, stream, s, v, in, idx, n, has_amb, ar,
                               ag, ab, st, colors, out);
        else
            hipLaunchKernelGGL((lights_primary_kernel<ST, AL, false>), grid, block, 0, stream, s, v, in, idx, n, has_amb, ar,
                               ag, ab, st, colors, out);
    });
    return hipGetLastError();
}

hipError_t launch_light_term(int store, int algo, const KScene& s, const KView& v, const uint32_t* idx, uint32_t n,
                             const void* state, uint32_t* colors, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const dim3 grid((n + kLightsThreads - 1u) / kLightsThreads), block(kLightsThreads);
    const uint4* st = static_cast<const uint4*>(state);
    for_store_algo(store, algo, [&](auto sto, auto al) {
        constexpr int ST = decltype(sto)::value, AL = decltype(al)::value;
        hipLaunchKernelGGL((light_term_kernel<ST, AL>), grid, block, 0, stream, s, v, idx, n, st, colors);
    });
    return hipGetLastError();
}

}  // namespace vr
