// vr_march.hip -- the render path of the per-pixel voxel ray march for gfx950 (CDNA4):
// the tile pass (march_kernel), the crawl pass (crawl_kernel) and launch_march.
//
// One lane per pixel; one wave64 = one 8x8 pixel tile (the reference's 8x8
// CUDA block, Main.cu:109-111, but as a single wavefront so the tile's rays
// walk the same clusters together), two waves (tiles side by side) per
// 128-thread workgroup (kTilesX/kTilesY, vr_lane_order.h).  Templated on {store, algorithm, count}: no virtual calls, no
// function pointers (the reference's StorageStructure vtable,
// StorageStructure.cuh:12-56, and nextXFunc pointers, Renderer.cuh:263-265,
// become compile-time branches).
//
// The walks are the Walker of vr_walk.h (its arithmetic and FP policy: there).  The
// shadow ray of a hit is evaluated after the primary walk returns instead of
// from inside it (Renderer.cuh:315,737,821,...): the shadow result depends
// only on (hit origin, region, shadow algorithm), so the pixel is identical.
// The learned orders' kernels are vr_order.hip, pick and trace vr_query.hip, the small
// utility kernels vr_util.hip.
#include "vr_device.h"

#include <algorithm>
#include <type_traits>

// VR_DIAG (the counting build libvr_cover.so; profiles/wave_counts.py and
// tests/cover_run.py read it): wave-level execution counters -- one atomic per wave
// per counted event, from the wave's first active lane.  Never part of libvr.so.
// 0-25: the hot loops (profiles/wave_counts.py NAMES).  32-58: the rarely-taken blocks
// that keep the walks exact -- one beside every __builtin_expect site, the ray
// direction's fallback, every sign-pattern arm (VR_DIAG_PAT: primary 43 + pattern,
// shadow 51 + pattern), a wave's second pattern pass, pattern 7 through P,P,P --
// whose reach tests/test_gpu_edges.py::test_guards_are_reached proves (the table
// GUARDS of tests/cover_run.py names every index).
// This unit alone counts: it defines the macros before vr_walk.h, whose defaults are no-ops
// (the pick and trace kernels of vr_query.hip count nothing).
#ifdef VR_CRAWL_PROF
// per crawl record of the last crawl pass (profiles/crawl_prof.py): {shader cycles, plain
// loop iterations (bit 31: walked from the start), crawl_run calls that applied steps, their
// loop trips, start and end (s_memrealtime, 100 MHz), 0, 0}
__device__ unsigned int g_vr_crawl_prof[16384 * 8];
#endif
#ifdef VR_DIAG
__device__ unsigned long long g_vr_diag[64];
#define VR_DIAG_COUNT(k)                                                              \
    do {                                                                             \
        if (__lane_id() == (uint32_t)__builtin_ctzll(__builtin_amdgcn_read_exec())) \
            atomicAdd(&g_vr_diag[(k)], 1ull);                                        \
    } while (0)
#define VR_DIAG_COUNT_IF(c, k)                                  \
    do {                                                       \
        if (__builtin_amdgcn_ballot_w64(c) != 0) VR_DIAG_COUNT(k); \
    } while (0)
#define VR_DIAG_PAT(shadow, p) VR_DIAG_COUNT(((shadow) ? 51 : 43) + (p))
#endif
#include "vr_walk.h"

namespace vr {
namespace {

// The tile group (column, row of kTilesX x kTilesY tiles) this tile-pass workgroup
// renders: the work order's entry (heaviest first, KView::order), or its grid position
// (a uniform load: SGPRs).
__device__ __forceinline__ void tile_group(const KView& v, uint32_t& bx, uint32_t& by) {
    bx = blockIdx.x;
    by = blockIdx.y;
    if (v.order) {
        const uint32_t t = v.order[blockIdx.y * gridDim.x + blockIdx.x];
        bx = t & 0xFFFFu;
        by = t >> 16;
    }
}

// The pixel (local column x, local row l) of this tile-pass lane.  Without a lane order
// (KView::perm null) wave w of tile group (bx, by) is the 8x8 tile (2 bx + w, by).  With one,
// the tile groups of a kLaneBlockX x kLaneBlockY pixel block share its pixels: they are dealt
// to the block's waves heaviest first (perm_kernel, from the walk lengths an earlier launch
// of the view recorded), so a wave's lanes walk about equally far and finish together --
// C2: 25 % fewer wave-iterations for the same per-lane work with 16x16 blocks, 32 % with
// 16x32 (the oracle's per-pixel counts, profiles/r05/lane_sort_sim.py).  Slot q of a block is wave
// w of its tile group (bx mod kLbX, by mod kLbY) in row-major order, q = 2 (tile group) + w;
// lane i of slot q renders pixel perm[block * kLanePixels + 64 q + i] = (row * kLaneBlockX +
// column) of the block.  Blocks cut by the grid's edge keep the 8x8 tiles.
__device__ __forceinline__ void lane_pixel(const KView& v, uint32_t& x, uint32_t& l) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t bx, by;
    tile_group(v, bx, by);
    const uint32_t BX = bx / kLbX, BY = by / kLbY;
    if (kLaneOrder && v.perm && (BX + 1u) * kLbX <= gridDim.x && (BY + 1u) * kLbY <= gridDim.y) {
        const uint32_t q = ((by % kLbY) * kLbX + bx % kLbX) * kTilesX + wave;
        const uint32_t blk = BY * ((gridDim.x + kLbX - 1u) / kLbX) + BX;
        const uint32_t p = reinterpret_cast<const PermT*>(v.perm)[(size_t)blk * kLanePixels + q * 64u + lane];
        x = BX * kLaneBlockX + p % kLaneBlockX;
        l = BY * kLaneBlockY + p / kLaneBlockX;
    } else {
        x = (bx * kTilesX + wave % kTilesX) * 8u + (lane & 7u);
        l = (by * kTilesY + wave / kTilesX) * 8u + (lane >> 3);
    }
}

// The primary walk's length per tile-pass thread, for a launch that records the lane order's
// walk lengths (KView::pcost): shade writes it between the walks, march_kernel reads it back.
__device__ __forceinline__ uint32_t* tile_prim() {
    __shared__ uint32_t p[64u * kTilesX * kTilesY];
    return p;
}

// (light_and_shadow, the pixel's colour at a primary hit: vr_walk.h -- vr_shade.hip's kernel shares it)

// Tile pass: hand this lane's pixel (tile_pixels) to the crawl pass, to be walked there
// from its start (a record with flag 4).  Returns what the tile pass writes for
// it: 0, or kDeferMarker when the list is full (the crawl pass then finds the
// pixel by the marker).
__device__ __forceinline__ uint32_t defer_rewalk(const KView& v) {
    const uint32_t idx = atomicAdd(v.defer, 1u);
    deferral_report(v);
    if (idx < v.defer_cap) {
        uint32_t* r = v.defer + 4 + (size_t)idx * kDeferRecWords;
        r[0] = tile_pixels()[threadIdx.x];
        r[1] = 4u;
        r[8] = v.launch_id;
        return 0u;
    }
    atomicAdd(v.defer + 2, 1u);
    return kDeferMarker;
}

// The crawl pass's cluster bits for one record lane: its LDS slot, or (no slot: more records
// per wave than kCrawlMaxRpw) the scene's bits in memory for the crawls' closed form alone.
struct CrawlLds {
    uint32_t* lbm = nullptr;
    bool mem = false;
};
template <class W>
__device__ __forceinline__ void attach(W& w, const CrawlLds* cl) {
    if (!cl) return;
    w.lbm = cl->lbm;
    w.mem_bits = cl->mem;
}

// The body of rayMarchSceneOriginal / rayMarchSceneJumpAxis (Renderer.cuh:1033-1063)
// for pixel (x, local row l): colour, algorithmic bytes (+4 for the pixel write).
// Tile pass (!CRAWL): a pixel deferred to the crawl pass -- a crawl record, or a
// walk longer than kTileBudget iterations -- comes back with 0 bytes (the crawl
// pass writes and counts it).  Crawl pass: a walk that never finishes (the
// reference would loop forever) is 0 with only the pixel write counted, as in
// the oracle.
template <int STORE, int ALGO, bool COUNT, bool CRAWL>
__device__ __forceinline__ uint32_t shade(const KScene& s, const KView& v, uint32_t x, uint32_t l,
                                          uint32_t& bytes, uint32_t* iters = nullptr, uint2* ff = nullptr,
                                          uint32_t* dg = nullptr, const CrawlLds* cl = nullptr) {
    uint32_t col = 0;
    bytes = 0;
    if (ff) *ff = uint2{0u, 0u};
    f3 ro, rd;
    if (pixel_ray<true>(v, x, l, ro, rd)) {
        Walker<STORE, COUNT, CRAWL> w(s, v);
        attach(w, cl);
        Hit h;
        const bool hit = w.template primary<ALGO>(ro, rd, h);
        if (!CRAWL && v.pcost) tile_prim()[threadIdx.x] = w.iters;   // (the lane order's primary walk length)
        if (hit) col = light_and_shadow<ALGO>(w, v, h);
        if (iters) *iters = w.iters;              // the walk's length (the work order's cost)
        bytes = w.bytes + 4u;                     // + the pixel write
        if (ff) *ff = uint2{w.ff, w.nl};
#ifdef VR_CRAWL_PROF
        if (dg) { dg[0] = w.iters - w.ff; dg[1] = w.d_runs; dg[2] = w.d_trips; }
#endif
        if (w.aborted) {
            col = 0;
            if (ff) *ff = uint2{0u, 0u};
            if (Walker<STORE, COUNT, CRAWL>::kExact) {
                bytes = 4u;
            } else {
                bytes = 0u;
                if (w.iters != kDeferredIters) col = defer_rewalk(v);
            }
        }
    }
    return col;
}

// The crawl pass's pixel: the walk a deferral record `r` left at its crawl,
// finished from there (its iterations and bytes so far are the record's).
template <int STORE, int ALGO, bool COUNT>
__device__ __forceinline__ uint32_t shade_resume(const KScene& s, const KView& v,
                                                 const uint32_t* r, uint32_t& bytes, uint2& ff,
                                                 uint32_t* dg = nullptr, const CrawlLds* cl = nullptr) {
    const uint32_t x = r[0] & 0xFFFFu, l = r[0] >> 16;
    Walker<STORE, COUNT, true> w(s, v);
    attach(w, cl);
    w.iters = r[9];
    w.bytes = r[10];
    const f3 o{__uint_as_float(r[2]), __uint_as_float(r[3]), __uint_as_float(r[4])};
    const i3 cr{(int32_t)r[5], (int32_t)r[6], (int32_t)r[7]};
    uint32_t col = 0;
    if (!(r[1] & 1u)) {                           // the primary walk crawled
        f3 ro, rd;
        pixel_ray<true>(v, x, l, ro, rd);
        Hit h;
        if (w.template primary_regions<ALGO>(o, rd, cr, h, r)) col = light_and_shadow<ALGO>(w, v, h);
    } else {                                      // the shadow walk crawled
        const bool eq = v.L[0] == v.L[1] && v.L[1] == v.L[2];
        bool sh;
        if (r[1] & 2u) sh = eq ? w.template shadow<true, true>(o, cr, r) : w.template shadow<true>(o, cr, r);
        else sh = eq ? w.template shadow<false, true>(o, cr, r) : w.template shadow<false>(o, cr, r);
        col = r[18] * (uint32_t)!sh;
    }
    bytes = w.bytes + 4u;
    ff = uint2{w.ff, w.nl};
#ifdef VR_CRAWL_PROF
    if (dg) { dg[0] = w.iters - r[9] - w.ff; dg[1] = w.d_runs; dg[2] = w.d_trips; }
#endif
    if (w.aborted) {                              // never finishes (see shade)
        col = 0;
        bytes = 4u;
        ff = uint2{0u, 0u};
    }
    return col;
}

__device__ __forceinline__ void add_bytes(const KView& v, uint32_t lane, unsigned long long b) {
    for (int off = 32; off > 0; off >>= 1) b += __shfl_down(b, off, 64);   // one atomic per wave
    if (lane == 0 && b) atomicAdd(v.bytes, b);
}
// the crawl pass's existence reads credited without a load (KView::stats): n crawl
// iterations fast-forwarded in closed form, m skip steps answered from the LDS cluster bits
__device__ __forceinline__ void add_ff(const KView& v, uint32_t lane, unsigned long long n, unsigned long long m) {
    for (int off = 32; off > 0; off >>= 1) {
        n += __shfl_down(n, off, 64);
        m += __shfl_down(m, off, 64);
    }
    if (lane == 0 && (n | m) && v.stats) {
        atomicAdd(v.stats, n);
        atomicAdd(v.stats + 1, 4ull * (n + m));
    }
}

// Tile pass: one lane per pixel, one wave per 8x8 tile, kTilesX x kTilesY tiles per workgroup.
#ifndef VR_ORIG_WAVES
#define VR_ORIG_WAVES 7
#endif
#ifndef VR_LONG_WAVES
#define VR_LONG_WAVES 6
#endif
// HI: the occupancy for frames in flight, where the other frame's waves fill the tail and
// the pass's throughput counts: one wave per SIMD more for the cuckoo walk (latency-bound
// on its random slot loads: C4 0.0861 -> 0.0855 ms per frame, but 0.1229 -> 0.1246 alone)
// and the longest-axis walk (C3 0.2311 -> 0.2289 per frame, 0.2815 -> 0.2862 alone),
// profiles/r04/ab_orig_waves_C4.txt, ab_long_waves_C3.txt.  The host picks HI for a launch
// whose device is still running another stream's (the AUTO schedule's test).
// (Round 6: 7 for the cuckoo walk too.  Since its shadow walks answer a hit from the filter
// alone -- no table reads -- the 8-wave variant's SGPRs spill into VGPR lanes, 16 v_readlane
// per loop iteration: C4 per frame in flight 0.0500 -> 0.0746 ms at 8 waves, 0.0466 at 7,
// profiles/r06/ab_C4_*.txt.)
#ifndef VR_ORIG_WAVES_HI
#define VR_ORIG_WAVES_HI 7
#endif
// (Round 6: 6 for the VCS longest-axis walk too, the lone kernel's, so frames in flight run
// that kernel.  With its shadow direction in VGPRs and the direction made per region round
// the 7-wave variant spills 30 VGPRs and 212 SGPRs: C3 per frame in flight 0.1851 -> 0.1835 ms
// at 6, profiles/r06/ab/ab_C3_waves_hi.txt.)
#ifndef VR_LONG_WAVES_HI
#define VR_LONG_WAVES_HI 6
#endif
// (a variant equal to the lone one is not built: launch_march names march_kernel<..., true>
// only through kHiVariant, so a pair without one launches -- and instantiates -- the lone kernel)
constexpr bool kLongHiVariant = VR_LONG_WAVES_HI != VR_LONG_WAVES;
constexpr bool kOrigHiVariant = VR_ORIG_WAVES_HI != VR_ORIG_WAVES;
// (the in-flight occupancy variants exist for the uninstrumented cuckoo original and
// VCS longest-axis walks; the VCS original walk is fastest at 7 waves either way)
template <int STORE, int ALGO>
constexpr bool kHiVariant = (STORE == STORE_VCS && ALGO == ALGO_LONGEST && kLongHiVariant) ||
                            (STORE == STORE_HASH && ALGO == ALGO_ORIGINAL && kOrigHiVariant);
template <int ALGO, bool HI> struct TileWaves {
    static constexpr int value = ALGO == ALGO_ORIGINAL ? (HI ? VR_ORIG_WAVES_HI : VR_ORIG_WAVES)
                                                       : (HI ? VR_LONG_WAVES_HI : VR_LONG_WAVES);
};
static_assert(kTilesX * kTilesY == kWavesPerTileGroup, "cost layout (vr_internal.h)");
template <int STORE, int ALGO, bool COUNT, bool HI = false>
__global__ __launch_bounds__(64 * kTilesX * kTilesY, (TileWaves<ALGO, HI>::value)) void march_kernel(KScene s, KView v) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t x, l;
    lane_pixel(v, x, l);
    tile_pixels()[threadIdx.x] = (l << 16) | x;     // (read back only by this lane: no barrier)
    if (v.pcost) tile_prim()[threadIdx.x] = 0u;
    uint32_t bytes = 0, iters = 0;
    if (x < v.LW && l < v.local_rows) {
        // (&iters unconditionally: a pointer chosen by `v.cost ? &iters : nullptr` keeps
        // iters in scratch -- a store and a reload per lane, 8 MB of WRITE_SIZE per C2 launch)
        const uint32_t c = shade<STORE, ALGO, COUNT, false>(s, v, x, l, bytes, &iters);
        // (x and l again from LDS, so they are not live through the walk; the empty asm
        // keeps the compiler from forwarding the stored value instead)
        asm volatile("" ::: "memory");
        const uint32_t p = tile_pixels()[threadIdx.x];
        const size_t at = (size_t)(p >> 16) * v.LW + (p & 0xFFFFu);
        v.out[at] = c;
        if (v.pcost) {                            // the pixel's walk lengths, for the next lane order
            // A pixel handed to the crawl pass (shade: 0 bytes after a walk) stores the half that
            // was walking saturated, however it was handed over: a crawl record leaves
            // kDeferredIters in iters, a longest-axis jump crawl and a walk past the budget their
            // count so far.  (No shadow iterations yet: the primary walk was the one.)
            const uint32_t p0 = tile_prim()[threadIdx.x];
            const bool deferred = bytes == 0u && iters != 0u;
            const uint32_t pp = deferred && iters == p0 ? 0xFFFFu : min(p0, 0xFFFFu);
            const uint32_t ss = deferred && iters != p0 ? 0xFFFFu : min(iters - p0, 0xFFFFu);
            v.pcost[at] = pp << 16 | ss;
        }
    }
    if (COUNT) add_bytes(v, lane, bytes);
    if (v.cost) {                                  // the wave's walk length, for the next work order
        for (int off = 32; off > 0; off >>= 1) iters = max(iters, (uint32_t)__shfl_xor((int)iters, off, 64));
        if (lane == 0) {
            uint32_t bx, by;
            tile_group(v, bx, by);
            v.cost[(by * gridDim.x + bx) * kWavesPerTileGroup + wave] = iters;
        }
    }
}

// Crawl pass: the deferred pixels of this launch, one per lane, with the
// exact crawl fast-forward; the last workgroup resets the slot for reuse.
#ifndef VR_CRAWL_RPW
#define VR_CRAWL_RPW 4
#endif
constexpr uint32_t kCrawlRpw = VR_CRAWL_RPW;
#ifndef VR_CRAWL_MAX_RPW
#define VR_CRAWL_MAX_RPW 32
#endif
constexpr uint32_t kCrawlMaxRpw = VR_CRAWL_MAX_RPW;     // records per wave with an LDS bitmap slot
// Workgroup shape: 2 waves (as the tile pass).  (Round 4 measured an opt-in mode that cached
// the scene's whole region table and cluster bits in each 8-wave workgroup's LDS: no faster
// alone, slower in flight, profiles/r04/crawl/scene_lds_ab.txt -- removed in round 5.)
constexpr uint32_t kCrawlWaves = 2;
// LDS (16-B aligned carve-outs, cdna_hip_programming.md Guideline 17):
//   [0, 16)   record count, overflow count
//   then      16 words (a region's cluster-existence bits) per record lane, kCrawlMaxRpw per wave
constexpr uint32_t kCrawlLdsWords = 4u + kCrawlWaves * kCrawlMaxRpw * 16u;
template <int STORE, int ALGO, bool COUNT>
__global__ __launch_bounds__(64 * kCrawlWaves) void crawl_kernel(KScene s, KView v) {
    __shared__ __attribute__((aligned(16))) uint32_t dyn[kCrawlLdsWords];
    if (threadIdx.x == 0) {
        dyn[0] = v.defer[0];
        dyn[1] = v.defer[2];
    }
    __syncthreads();
    const uint32_t total = dyn[0], overflow = dyn[1];
    // what this launch deferred, for the host's grid size of later launches (a hint only)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (v.defer_stat) *v.defer_stat = total + overflow;
        if (v.slot_stat) *reinterpret_cast<uint2*>(v.slot_stat) = uint2{v.launch_id, total + overflow};
    }
    if (total == 0u && overflow == 0u) return;   // nothing deferred (the usual case): no reset needed
    const uint32_t n = min(total, v.defer_cap);
    CrawlLds cl;
    unsigned long long bytes = 0, ffs = 0, nls = 0;
    // kCrawlRpw records per wave at a time (lanes 0 .. kCrawlRpw-1): each record is a long
    // chain of dependent iterations, and the lanes of a wave take different paths through
    // the walk, so fewer lanes per wave -- spread over more waves -- finish sooner
    // (v.crawl_rpw: the host's choice per launch, vr_launch_plan.h launch_policy -- 2 for a
    // lone frame, whose time is the longest record's chain; VR_CRAWL_RPW_IN_FLIGHT, 32 by
    // default, with frames in flight, where the pass's issue cycles count; VR_CRAWL_RPW = 1..64
    // for every launch.  Above kCrawlMaxRpw no lane has an LDS slot: every skip step loads,
    // and the crawls' closed form reads the cluster bits from memory.
    // Round 3 ran 4 and 8: C5 0.6707 -> 0.6514 ms per frame in flight, profiles/r03/rpw_deep/)
    const uint32_t rpw = v.crawl_rpw ? v.crawl_rpw : kCrawlRpw;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, wlane = threadIdx.x & 63u;
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    if (STORE == STORE_VCS && s.vcs_cbits && wlane < rpw) {
        if (rpw <= kCrawlMaxRpw) cl.lbm = dyn + 4 + ((threadIdx.x >> 6) * kCrawlMaxRpw + wlane) * 16u;
        else cl.mem = true;
    }
    for (uint32_t i = wave * rpw + wlane; wlane < rpw && i < n; i += nwaves * rpw) {
        uint32_t* r = v.defer + 4 + (size_t)i * kDeferRecWords;
        // (a record of another launch -- one whose crawl pass the host skipped, believing its
        // view defers nothing -- is not this frame's: never shade it into this frame; its count
        // in this pass's report stops the skipping)
        if (r[8] != v.launch_id) continue;
        uint32_t b;
        const uint32_t x = r[0] & 0xFFFFu, l = r[0] >> 16;
        // The crawl iteration's voxel q (see crawl_voxel), recovered from the stepped
        // position and the walk's direction (the pixel's ray, or the light for a shadow
        // walk) into record words 15-17; if it cannot be, the pixel is walked from its
        // start (as for every record under VR_KERNEL_TILE_REWALK, flag 4).
        bool amb = (r[1] & 4u) != 0u;
        if (!amb) {
            f3 d = ld3(v.L);
            if (!(r[1] & 1u)) {
                f3 ro;
                pixel_ray<true>(v, x, l, ro, d);
            }
            const f3 o{__uint_as_float(r[2]), __uint_as_float(r[3]), __uint_as_float(r[4])};
#pragma unroll 1
            for (uint32_t a = 0; a < 3u; ++a) {
                int32_t qa;
                amb |= !crawl_voxel(comp(o, a), kEps * comp(d, a), qa);
                r[15 + a] = (uint32_t)qa;
            }
        }
        uint2 f{0u, 0u};
#ifdef VR_CRAWL_PROF
        uint32_t dg[3] = {0, 0, 0};
        const long long c0 = clock64(), t0 = wall_clock64();
        v.out[(size_t)l * v.LW + x] = amb ? shade<STORE, ALGO, COUNT, true>(s, v, x, l, b, nullptr, &f, dg, &cl)
                                         : shade_resume<STORE, ALGO, COUNT>(s, v, r, b, f, dg, &cl);
        const long long c1 = clock64(), t1 = wall_clock64();
        if (i < 16384u) {
            g_vr_crawl_prof[8 * i + 0] = (uint32_t)min(c1 - c0, 0xFFFFFFFFll);
            g_vr_crawl_prof[8 * i + 1] = dg[0] | (amb ? 0x80000000u : 0u);
            g_vr_crawl_prof[8 * i + 2] = dg[1];
            g_vr_crawl_prof[8 * i + 3] = dg[2];
            g_vr_crawl_prof[8 * i + 4] = (uint32_t)t0;
            g_vr_crawl_prof[8 * i + 5] = (uint32_t)t1;
        }
#else
        v.out[(size_t)l * v.LW + x] = amb ? shade<STORE, ALGO, COUNT, true>(s, v, x, l, b, nullptr, &f, nullptr, &cl)
                                         : shade_resume<STORE, ALGO, COUNT>(s, v, r, b, f, nullptr, &cl);
#endif
        bytes += b;
        ffs += f.x;
        nls += f.y;
    }
    if (overflow != 0u) {
        // the list overflowed: the pixels the tile pass could not defer carry the marker
        const size_t npx = (size_t)v.local_rows * v.LW;
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npx; i += (size_t)gridDim.x * blockDim.x) {
            if (v.out[i] != kDeferMarker) continue;
            uint32_t b;
            uint2 f{0u, 0u};
            // (a per-record bit slot is not this lane's: none)
            const CrawlLds clo;
            v.out[i] = shade<STORE, ALGO, COUNT, true>(s, v, (uint32_t)(i % v.LW), (uint32_t)(i / v.LW), b, nullptr, &f,
                                                       nullptr, &clo);
            bytes += b;
            ffs += f.x;
            nls += f.y;
        }
    }
    if (COUNT) {
        add_bytes(v, threadIdx.x & 63u, bytes);
        add_ff(v, threadIdx.x & 63u, ffs, nls);
    }
    // Every workgroup has read the count (above) before it adds to `done`; the
    // last one clears the slot for its next launch (ordered by the kernel boundary).
    __syncthreads();
    if (threadIdx.x == 0 && atomicAdd(&v.defer[1], 1u) == gridDim.x - 1u) {
        v.defer[0] = 0;
        v.defer[1] = 0;
        v.defer[2] = 0;
    }
}

}  // namespace

// The tile pass, then the crawl pass (a small grid that exits at once when nothing
// was deferred), both on `stream`.  (The crawl pass on a high-priority side stream,
// fenced by events, measured slower on every config: C2 0.1148 -> 0.1224 ms per frame
// with two in flight, 0.154 -> 0.184 alone; profiles/r03/ab_crawl_stream.txt.)
// The crawl pass's grid: kCrawlRpw records per wave, all of them at once (each record is
// a latency-bound chain: C5 rpw 64 / 16 / 8 / 4 -> 0.93 / 0.82 / 0.80 / 0.76 ms per frame in
// flight, profiles/r03/ab_crawl_rpw.txt), at least 64 workgroups.  The host sizes it from
// the count an earlier launch of the device wrote to defer_stat: a launch that defers
// nothing (C2-C4) keeps the small grid (1024 empty workgroups cost C2 0.6 %).
uint32_t crawl_grid(uint32_t records, uint32_t rpw) {
    const uint32_t waves_per_wg = kCrawlWaves;
    rpw = rpw ? rpw : kCrawlRpw;
    const uint64_t waves = ((uint64_t)records * 5u / 4u + rpw - 1u) / rpw;
    const uint64_t wgs = (waves + waves_per_wg - 1u) / waves_per_wg;
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(wgs, 64u), 4096u);
}

// VR_NO_CRAWL_PASS: a measurement-only build without the crawl pass (its cost on a
// frame that defers nothing, C2: profiles/r03/ab_no_crawl_pass_C2.txt); wrong for any
// frame that defers a pixel.
#ifdef VR_NO_CRAWL_PASS
constexpr bool kNoCrawlPass = true;
#else
constexpr bool kNoCrawlPass = false;
#endif

void march_grid(const KView& v, uint32_t& columns, uint32_t& rows) {
    columns = (v.LW + 8u * kTilesX - 1u) / (8u * kTilesX);
    rows = (v.local_rows + 8u * kTilesY - 1u) / (8u * kTilesY);
}

namespace {
// One tile pass, then its crawl pass.  HI: the in-flight occupancy variant of the tile pass;
// callers pass it only where kHiVariant says one exists.
struct MarchLaunch {
    dim3 grid, block, cgrid, cblock;
    hipStream_t stream;
    bool crawl;
    template <int ST, int AL, bool CT, bool HI>
    void run(const KScene& s, const KView& v) const {
        hipLaunchKernelGGL((march_kernel<ST, AL, CT, HI>), grid, block, 0, stream, s, v);
        if (v.defer && crawl && !kNoCrawlPass)
            hipLaunchKernelGGL((crawl_kernel<ST, AL, CT>), cgrid, cblock, 0, stream, s, v);
    }
};
}  // namespace

hipError_t launch_march(int store, int algo, bool count, const KScene& s, const KView& v, hipStream_t stream,
                        uint32_t crawl_wgs, bool in_flight, bool crawl) {
    uint32_t gx, gy;
    march_grid(v, gx, gy);
    if (gx == 0 || gy == 0) return hipSuccess;
    const MarchLaunch m{dim3(gx, gy), dim3(64u * kTilesX * kTilesY), dim3(crawl_wgs ? crawl_wgs : 64u),
                        dim3(64u * kCrawlWaves), stream, crawl};
#ifdef VR_ISA_ONLY
    // ISA-inspection builds (csrc/Makefile isa1, profiles/loop_isa.py): one kernel pair
    // only, e.g. -DVR_ISA_ONLY=ALGO_LONGEST for the VCS longest-axis tile pass; never a library
    // (-DVR_ISA_STORE=STORE_HASH for a cuckoo pair, with its in-flight variant)
#ifndef VR_ISA_STORE
#define VR_ISA_STORE STORE_VCS
#endif
    (void)algo; (void)count; (void)store;
    if (in_flight) m.run<VR_ISA_STORE, VR_ISA_ONLY, false, true>(s, v);
    else m.run<VR_ISA_STORE, VR_ISA_ONLY, false, false>(s, v);
#else
    for_store_algo(store, algo, [&](auto st, auto al) {
        constexpr int ST = decltype(st)::value, AL = decltype(al)::value;
        if (count) m.run<ST, AL, true, false>(s, v);
        else if (in_flight) m.run<ST, AL, false, kHiVariant<ST, AL>>(s, v);   // (no variant: the lone kernel)
        else m.run<ST, AL, false, false>(s, v);
    });
#endif
    return hipGetLastError();
}

}  // namespace vr

#ifdef VR_CRAWL_PROF
extern "C" int vr_crawl_prof_fetch(unsigned int* out, unsigned int n) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_vr_crawl_prof), sizeof(unsigned int) * 8 * (n < 16384u ? n : 16384u)) !=
        hipSuccess)
        return -1;
    return 0;
}
#endif
#ifdef VR_DIAG
// The 64 counters (the device the calling thread has current), optionally zeroed after the
// read.  Only the counting build has it: it is no part of include/vr.h.
extern "C" int vr_diag_fetch(uint64_t* out, int reset) {
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "counter width");
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_vr_diag), sizeof(unsigned long long) * 64) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[64] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_vr_diag), z, sizeof z) != hipSuccess) return -1;
    }
    return 0;
}
#endif
