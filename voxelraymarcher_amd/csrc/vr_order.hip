// vr_order.hip -- the learned orders of the tile pass (vr_march.hip): perm_kernel makes a
// view's lane order (which pixel each lane of a pixel block renders, KView::perm) from the walk
// lengths an earlier launch recorded, order_kernel its work order (heaviest tile groups
// first, KView::order).  The shapes both share with lane_pixel: vr_lane_order.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vr_internal.h"
#include "vr_lane_order.h"

namespace vr {
namespace {

// The lane order of one pixel block (see lane_pixel): its kLanePixels pixels ranked by the
// walk length an earlier launch recorded (KView::pcost), heaviest first, one thread per pixel.
// Keys (length << log2(kLanePixels) | pixel) are all distinct.  Each wave sorts its 64 keys
// with a bitonic network of lane shuffles (no barriers); a key's rank in the block is its
// rank in its wave plus, for each other wave, the number of that wave's sorted keys above it
// (independent binary searches in LDS).  The block's slots are gathered in LDS and stored as
// words.  With cost non-null the kernel also writes each wave's walk length under the new
// lane order -- KView::cost's layout; max(primary) + max(shadow) over the wave's pixels, what
// the wave runs; blocks cut by the grid's edge keep the 8x8 tiles and write each tile's -- so
// the work order made from them next matches the lane order.
// With kLaneSeat == 1 each wave then sorts the 64 pixels of its own slot once more, by the
// Morton code of (column, row) ascending (lane_morton): the slot's pixel set, and with it
// wmax and cost, is what the cost ranks made it; only the lanes within the slot change.
// A wave's 64 keys sorted by a bitonic network of lane shuffles: lane i gets the i-th largest
// (DESCENDING) or the i-th smallest.
template <bool DESCENDING>
__device__ __forceinline__ uint32_t wave_sort(uint32_t key, uint32_t lane) {
    for (uint32_t size = 2; size <= 64u; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            const uint32_t other = (uint32_t)__shfl_xor((int)key, (int)stride, 64);
            const bool keep_max = (((lane & stride) == 0u) == ((lane & size) == 0u)) == DESCENDING;
            key = keep_max ? max(key, other) : min(key, other);
        }
    }
    return key;
}
// The Morton code of block pixel (px, py): bit 2i is bit i of the column, bit 2i + 1 bit i of
// the row, for the low four bits of each; a fifth bit of the column (32 wide) is bit 8, of the
// row (32 high) bit 9.
__device__ __forceinline__ uint32_t lane_morton(uint32_t px, uint32_t py) {
    auto spread4 = [](uint32_t v) {
        v = (v | v << 2) & 0x33u;
        return (v | v << 1) & 0x55u;
    };
    return spread4(px & 15u) | spread4(py & 15u) << 1 | (px >> 4) << 8 | (py >> 4) << 9;
}
__global__ __launch_bounds__(kLanePixels) void perm_kernel(const uint32_t* __restrict__ pcost, uint32_t LW,
                                                           uint32_t rows, uint32_t gx, uint32_t gy,
                                                           uint8_t* __restrict__ perm, uint32_t* __restrict__ cost) {
    constexpr uint32_t kWaves = kLanePixels / 64u, kTiles = (kLaneBlockX / 8u) * (kLaneBlockY / 8u);
    __shared__ uint32_t sorted[kLanePixels];
    __shared__ __attribute__((aligned(16))) PermT slots[kLanePixels];
    __shared__ uint32_t wmax[2u * kWaves];   // per wave slot (or 8x8 tile): max primary, max shadow
    __shared__ uint32_t ps[kLanePixels];     // the pixels' walk lengths (cost writes only)
    static_assert(kTiles == kWaves, "one 8x8 tile per wave slot");
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t nbx = (gx + kLbX - 1u) / kLbX, BX = blockIdx.x % nbx, BY = blockIdx.x / nbx;
    const uint32_t px = t % kLaneBlockX, py = t / kLaneBlockX;
    const uint32_t x = BX * kLaneBlockX + px, l = BY * kLaneBlockY + py;
    // a pixel's weight: a wave runs its primary walks until the slowest ends, then its shadow
    // walks, so it costs max(primary) + max(shadow) over its lanes; max(p, s) + (p + s) / 8
    // groups lanes best of the weights tried on the oracle's C2 counts (1.4 % fewer
    // wave-iterations than p + s, profiles/r05/lane_sort_sim.py)
    uint32_t p = 0, s = 0;
    if (x < LW && l < rows) {
        const uint32_t w = pcost[(size_t)l * LW + x];
        p = w >> 16;
        s = w & 0xFFFFu;
    }
    const uint32_t c = min(max(p, s) + ((p + s) >> 3), (1u << (32u - kLaneShift)) - 1u);
    if (cost) {
        if (t < 2u * kWaves) wmax[t] = 0u;
        ps[t] = p << 16 | s;
    }
    if ((BX + 1u) * kLbX > gx || (BY + 1u) * kLbY > gy) {
        if (cost) {                 // the block's 8x8 tiles that exist
            __syncthreads();
            const uint32_t ti = (py >> 3) * (kLaneBlockX / 8u) + (px >> 3);
            atomicMax(&wmax[ti], p);
            atomicMax(&wmax[kWaves + ti], s);
            __syncthreads();
            if (t < kTiles) {
                const uint32_t tx = t % (kLaneBlockX / 8u), ty = t / (kLaneBlockX / 8u);
                const uint32_t col = BX * kLbX + tx / kTilesX, row = BY * kLbY + ty;
                if (col < gx && row < gy)
                    cost[(row * gx + col) * kWavesPerTileGroup + tx % kTilesX] = wmax[t] + wmax[kWaves + t];
            }
        }
        return;
    }
    const uint32_t key = wave_sort<true>((c << kLaneShift) | t, lane);
    sorted[t] = key;                // lane i of wave w: the wave's i-th largest key
    __syncthreads();
    uint32_t rank = lane;
#pragma unroll
    for (uint32_t o = 1; o < kWaves; ++o) {
        const uint32_t* sw = sorted + (((wave + o) % kWaves) << 6);
        uint32_t lo = 0;            // the number of sw's keys above key (sw descending)
#pragma unroll
        for (uint32_t step = 32; step > 0; step >>= 1)
            if (sw[lo + step - 1u] > key) lo += step;
        rank += lo + (sw[63] > key ? 1u : 0u);    // (all 64 above: lo stops at 63)
    }
    const uint32_t pix = key & (kLanePixels - 1u);
    slots[rank] = (PermT)pix;
    if (cost) {                     // the walk lengths of the pixel this thread's key carries
        const uint32_t w = ps[pix];
        atomicMax(&wmax[rank >> 6], w >> 16);
        atomicMax(&wmax[kWaves + (rank >> 6)], w & 0xFFFFu);
    }
    __syncthreads();
    if (cost && t < kWaves) {
        const uint32_t g = t / kTilesX;
        const uint32_t col = BX * kLbX + g % kLbX, row = BY * kLbY + g / kLbX;
        cost[(row * gx + col) * kWavesPerTileGroup + t % kTilesX] = wmax[t] + wmax[kWaves + t];
    }
    if (kLaneSeat == 1u) {          // this wave's threads hold the 64 seats of slot `wave`
        const uint32_t q = slots[t];
        const uint32_t k = wave_sort<false>(lane_morton(q % kLaneBlockX, q / kLaneBlockX) << kLaneShift | q, lane);
        slots[t] = (PermT)(k & (kLanePixels - 1u));
        __syncthreads();
    }
    constexpr uint32_t kWords = kLanePixels * sizeof(PermT) / 4u;
    uint32_t* out = reinterpret_cast<uint32_t*>(perm + (size_t)blockIdx.x * kLanePixels * sizeof(PermT));
    if (t < kWords) out[t] = reinterpret_cast<const uint32_t*>(slots)[t];
}

// Heaviest tiles first: a counting sort of the tile groups by the cost an earlier
// launch recorded (the slower of a workgroup's waves; classes of 4 loop iterations,
// class 0 the heaviest, >= 508), in one workgroup with LDS counters.  The order within
// a class is whatever the atomics make it: any permutation renders the same pixels.
// (A stable sort -- grid order within a class, one ballot per class present per 64
// groups -- took ~4x longer and gained nothing, profiles/r03/ab_order_C2_C3.txt.)
constexpr uint32_t kOrderClasses = 128;
__global__ __launch_bounds__(1024) void order_kernel(const uint32_t* __restrict__ cost, uint32_t n, uint32_t columns,
                                                     uint32_t* __restrict__ order) {
    __shared__ uint32_t cnt[kOrderClasses];
    if (threadIdx.x < kOrderClasses) cnt[threadIdx.x] = 0u;
    __syncthreads();
    auto cls = [&](uint32_t i) {
        uint32_t c = 0;
#pragma unroll
        for (uint32_t w = 0; w < kWavesPerTileGroup; ++w) c = max(c, cost[i * kWavesPerTileGroup + w]);
        return kOrderClasses - 1u - min(kOrderClasses - 1u, c >> 2);
    };
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) atomicAdd(&cnt[cls(i)], 1u);
    __syncthreads();
    if (threadIdx.x == 0) {                        // exclusive prefix sum
        uint32_t run = 0;
        for (uint32_t k = 0; k < kOrderClasses; ++k) {
            const uint32_t c = cnt[k];
            cnt[k] = run;
            run += c;
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) order[atomicAdd(&cnt[cls(i)], 1u)] = (i / columns) << 16 | (i % columns);
}

}  // namespace

size_t perm_bytes(uint32_t gx, uint32_t gy) {
    return (size_t)((gx + kLbX - 1u) / kLbX) * ((gy + kLbY - 1u) / kLbY) * kLanePixels * sizeof(PermT);
}

LaneShape lane_shape() {
    return {kLaneBlockX, kLaneBlockY, (uint32_t)sizeof(PermT), kLaneSeat};
}

hipError_t launch_perm(const uint32_t* pcost, uint32_t LW, uint32_t rows, uint32_t gx, uint32_t gy, uint8_t* perm,
                       uint32_t* cost, hipStream_t stream) {
    const uint32_t nb = ((gx + kLbX - 1u) / kLbX) * ((gy + kLbY - 1u) / kLbY);
    if (nb == 0) return hipSuccess;
    hipLaunchKernelGGL(perm_kernel, dim3(nb), dim3(kLanePixels), 0, stream, pcost, LW, rows, gx, gy, perm, cost);
    return hipGetLastError();
}

hipError_t launch_order(const uint32_t* cost, uint32_t n, uint32_t columns, uint32_t* order, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(order_kernel, dim3(1), dim3(1024), 0, stream, cost, n, columns, order);
    return hipGetLastError();
}

}  // namespace vr
