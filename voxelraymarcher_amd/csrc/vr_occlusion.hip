// vr_occlusion.hip -- voxel ambient occlusion (include/vr.h vr_occlusion, vr_shade_lights_ao;
// DESIGN.md 4k): for a vr_hit record, how open the hit face is at the hit point, from the eight
// voxels around the cell in front of the face.  One lane per record; the arithmetic is
// vr_occlusion_math.h's, all integer after one fp32 subtraction per tangent axis; the occupancy
// reads are vr_locate.h's two stages.  A unit of its own, so that every other kernel is compiled
// exactly as before.  No LDS, no atomics, no walk.
#include "vr_locate.h"

#include "vr_occlusion_math.h"

namespace vr {
namespace {

constexpr uint32_t kAoThreads = 256;

__device__ __forceinline__ uint32_t pick3(int a, uint32_t x, uint32_t y, uint32_t z) { return a == 0 ? x : (a == 1 ? y : z); }

// ao of the record at rec (64 bytes, 16-byte aligned: four 16-byte loads; any bytes are taken).
// A record that is no VOXEL hit with a unit axis normal is open (255) and reads nothing of the
// scene.  Otherwise the eight neighbours' region entries are read -- eight independent loads,
// none waited for before all are issued -- then their eight presence words, likewise; a load is
// left out (predicated, the lane stays) only where there is nothing to read: a neighbour outside
// the frame, or in a null region.  Every address is in bounds for any int32 coordinates:
// cell_of() tests the frame, a region entry other than kNone names one of the scene's regions,
// and a word index is below 8192.
template <int STORE>
__device__ __forceinline__ uint32_t record_ao(const KScene& s, const uint4* __restrict__ rec) {
    const uint4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
    // r0 = {status, color, voxel.x, voxel.y}  r1 = {voxel.z, normal.x, normal.y, normal.z}
    // r2 = {region.x, region.y, region.z, point.x}  r3 = {point.y, point.z, reserved, reserved}
    const int a = ao_axis((int32_t)r1.y, (int32_t)r1.z, (int32_t)r1.w);
    const bool live = r0.x == kPickVoxel && a >= 0;
    const int u = ao_axis_u(a < 0 ? 0 : a), w = ao_axis_w(a < 0 ? 0 : a);
    // the plane cell p = voxel + normal (uint32: wraps)
    const uint32_t px = r0.z + r1.y, py = r0.w + r1.z, pz = r1.x + r1.w;
    VoxelCell cell[8];
    uint32_t slot[8], bits[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t du = (uint32_t)ao_du(j), dw = (uint32_t)ao_dw(j);
        const uint32_t x = px + (u == 0 ? du : 0u) + (w == 0 ? dw : 0u), y = py + (u == 1 ? du : 0u) + (w == 1 ? dw : 0u),
                       z = pz + (u == 2 ? du : 0u) + (w == 2 ? dw : 0u);
        cell[j] = cell_of(s, (int32_t)x, (int32_t)y, (int32_t)z);
        if (!live) cell[j].entry = kNone;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) slot[j] = cell[j].entry != kNone ? s.region_slot[cell[j].entry] : kNone;
#pragma unroll
    for (int j = 0; j < 8; ++j) bits[j] = slot[j] != kNone ? presence_word<STORE>(s, slot[j], cell[j].word) : 0u;
    uint32_t occ = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) occ |= ((bits[j] >> cell[j].bit) & 1u) << j;
    const uint32_t qu = ao_q(__uint_as_float(pick3(u, r2.w, r3.x, r3.y)), (int32_t)pick3(u, r0.z, r0.w, r1.x),
                             (int32_t)pick3(u, r2.x, r2.y, r2.z));
    const uint32_t qw = ao_q(__uint_as_float(pick3(w, r2.w, r3.x, r3.y)), (int32_t)pick3(w, r0.z, r0.w, r1.x),
                             (int32_t)pick3(w, r2.x, r2.y, r2.z));
    return live ? ao_value(occ, qu, qw) : kAoOpen;
}

// vr_occlusion: ao[i] of record i, one 4-byte store per lane (a wave's stores are one 256-byte run).
template <int STORE>
__global__ __launch_bounds__(kAoThreads) void occlusion_kernel(KScene s, const uint4* __restrict__ hits, uint32_t n,
                                                             uint32_t* __restrict__ ao) {
    const uint32_t i = blockIdx.x * kAoThreads + threadIdx.x;
    if (i >= n) return;
    ao[i] = record_ao<STORE>(s, hits + (size_t)i * 4u);
}

// vr_shade_lights_ao's pass over the records of its primary walk: colors[i] = scale_rgb(colors[i],
// ao_factor(ao, strength)) and, when ao_out is given, ao_out[i] = ao.  Ray i's record, colour and
// ao are all at index i, so the lanes need no execution order; launches on one stream are ordered
// and word i belongs to one lane, so the read-modify-write needs no atomics.  With strength 0 the
// factor is 255 and the colours are not touched (nor read).
template <int STORE>
__global__ __launch_bounds__(kAoThreads) void occlusion_apply_kernel(KScene s, const uint4* __restrict__ hits, uint32_t n,
                                                                   uint32_t strength, uint32_t* __restrict__ colors,
                                                                   uint32_t* __restrict__ ao_out) {
    const uint32_t i = blockIdx.x * kAoThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t ao = record_ao<STORE>(s, hits + (size_t)i * 4u);
    if (ao_out) ao_out[i] = ao;
    const uint32_t m = ao_factor(ao, strength);
    if (m != 255u) colors[i] = scale_rgb(colors[i], m);
}

}  // namespace

hipError_t launch_occlusion(int store, const KScene& s, const void* hits, uint32_t n, uint32_t* ao, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const dim3 grid((n + kAoThreads - 1u) / kAoThreads), block(kAoThreads);
    const uint4* in = static_cast<const uint4*>(hits);
    if (store == STORE_VCS) hipLaunchKernelGGL(occlusion_kernel<STORE_VCS>, grid, block, 0, stream, s, in, n, ao);
    else hipLaunchKernelGGL(occlusion_kernel<STORE_HASH>, grid, block, 0, stream, s, in, n, ao);
    return hipGetLastError();
}

hipError_t launch_occlusion_apply(int store, const KScene& s, const void* hits, uint32_t n, uint32_t strength,
                                  uint32_t* colors, uint32_t* ao_out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const dim3 grid((n + kAoThreads - 1u) / kAoThreads), block(kAoThreads);
    const uint4* in = static_cast<const uint4*>(hits);
    if (store == STORE_VCS)
        hipLaunchKernelGGL(occlusion_apply_kernel<STORE_VCS>, grid, block, 0, stream, s, in, n, strength, colors, ao_out);
    else
        hipLaunchKernelGGL(occlusion_apply_kernel<STORE_HASH>, grid, block, 0, stream, s, in, n, strength, colors, ao_out);
    return hipGetLastError();
}

}  // namespace vr
