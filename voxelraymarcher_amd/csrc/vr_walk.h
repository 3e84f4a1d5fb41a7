// vr_walk.h -- the Walker: both grid walks, the VCS longest-axis walk, primary and shadow,
// light_and_shadow (a hit's colour) and pixel_ray.  Included by every unit that walks a ray:
// vr_march.hip (the tile and crawl passes), vr_query.hip (pick and trace) and vr_shade.hip.
//
// Arithmetic follows the reference expression by expression (file:line in
// each function) under the FP policy of SURVEY.md 8(c): -ffp-contract=off,
// correctly rounded '/' and sqrtf, fminf/fmaxf, truncating saturating
// float->int with NaN -> 0, wrapping int arithmetic (-fwrapv).
//
// With the walker come the few things the tile pass's walker needs from the render path:
// kDeferredIters, deferral_report, tile_pixels and the deferral write inside
// grid_original_rt (compiled out for CRAWL = true, which is all vr_query.hip and vr_shade.hip
// instantiate).
//
// The counting macros VR_DIAG_COUNT, VR_DIAG_COUNT_IF and VR_DIAG_PAT are no-ops here unless
// the including unit defined them first.  Only vr_march.hip does (g_vr_diag lives there): in
// the counting build libvr_cover.so the tile and crawl passes count, the pick and trace
// kernels of vr_query.hip and the shade kernel of vr_shade.hip do not.
#pragma once
#include "vr_device.h"
#include "vr_crawl.h"        // crawl_steps, crawl_run, crawl_voxel
#include "vr_lane_order.h"   // kTilesX, kTilesY (tile_pixels)

#include <type_traits>

#ifndef VR_DIAG_COUNT
#define VR_DIAG_COUNT(k) do { } while (0)
#endif
#ifndef VR_DIAG_COUNT_IF
#define VR_DIAG_COUNT_IF(c, k) do { } while (0)
#endif
#ifndef VR_DIAG_PAT
#define VR_DIAG_PAT(shadow, p) do { } while (0)
#endif

namespace vr {
namespace {

// Direction-sign specialisation of the VCS loop: S = +1 / -1 a sign every lane
// of the wave shares, 0 = per lane.  plane_v is px ? ceilf(o) + EPSILON :
// floorf(o) - EPSILON (next_plane_fma's value); plane_c8 the cluster-skip offset.
template <int S> struct Sgn { static constexpr int value = S; };
template <int S>
__device__ __forceinline__ float plane_v(float o, float g, float ge) {
    if constexpr (S > 0) return ceilf(o) + kEps;
    else if constexpr (S < 0) return floorf(o) - kEps;
    else return next_plane_fma(o, g, ge);
}
template <int S>
__device__ __forceinline__ int32_t plane_c8(int32_t c8) {
    if constexpr (S > 0) return 8;
    else if constexpr (S < 0) return 0;
    else return c8;
}

// VR_UNIFORM_SKIP: the cluster-skip planes and their selects are computed only in
// wave-iterations where some lane stands in an absent cluster (one uniform branch on
// the ballot).  In C2, 61 % of the primary and 60 % of the shadow wave-iterations
// have no skipping lane (VR_DIAG counters 22-25, profiles/r02/wave_counts_C2_skip.txt):
// those run 51 VALU instead of 61.  C2 0.1172 -> 0.1113 ms per frame in flight,
// identical pixels; C5 (sparse: mostly skips) 0.688 -> 0.697 (profiles/r02/ab_uniform_skip_*.txt).
// A three-way form (voxel planes only when some lane does not skip, so they wait for the
// load) measured slower: C2 0.1112 -> 0.1147, C5 0.688 -> 0.694 (ab_uniform_skip3_*.txt).
#ifndef VR_UNIFORM_SKIP
#define VR_UNIFORM_SKIP 1
#endif
#ifndef VR_LONG_TAIL_GENERIC
#define VR_LONG_TAIL_GENERIC false
#endif
// VR_LONG_TAIL_EQ: the original-DDA tail of a longest-axis shadow walk takes the
// one-division loop when the light's components are equal (as the original
// algorithm's shadow walks do).  Measured neutral on C3 (0.2722 vs 0.2736 ms alone,
// profiles/r03/ab_la_signs_unit_C3.txt): off, the tail stays one loop.
#ifndef VR_LONG_TAIL_EQ
#define VR_LONG_TAIL_EQ 0
#endif

// VR_SHADOW_ARMS (the tile pass's original shadow walk, both stores): the light's sign pattern
// is uniform, so it is dispatched on once per shadow ray with scalar branches -- the ray's whole
// sequence of region walks runs inside the arm of its pattern (Walker::arms, shadow_regions)
// -- instead of once per region round inside grid_original_rt, and the arm's set-up is
// specialised like its loop.  C2 per frame in flight 0.0949 -> 0.0933 ms, SQ_INSTS_VALU per
// launch 7.46e7 -> 7.27e7, identical frames (profiles/setup/).  0: the dispatch per round, as
// the primary walk and the longest-axis walks' tails keep it -- the same arms around the
// primary walk, where the pattern differs per lane, measured slower.
#ifndef VR_SHADOW_ARMS
#define VR_SHADOW_ARMS 1
#endif
// What an arm's region walks share, made once per ray: nlim = 2^-90 where the direction's
// three reciprocals are in div_fast's domain and no component is a guarded zero (walk_ok),
// else +inf; okw = every lane that entered the arm has walk_ok (uniform).
struct ArmRay {
    float nlim;
    bool okw;
};

// The iteration count of a tile-pass walk that wrote a crawl record (see the deferral
// in grid_original_rt): the pixel is the crawl pass's already.
constexpr uint32_t kDeferredIters = 0xFFFFFFFFu;

// A tile-pass lane that defers its pixel tells the host, through the launch slot's
// host-mapped report word (KView::slot_stat): {launch id, 1}.  On a launch that runs its
// crawl pass the pass overwrites it with its own count.  On a launch whose crawl pass the
// host skipped -- believing the view defers nothing -- it is the only writer, and the host
// stops skipping when it sees it (vr_launch_plan.h CrawlSkip): the next launch of the slot runs the
// crawl pass, which drops the stale records and resets the list.  (Rare: one 8-B store.)
__device__ __forceinline__ void deferral_report(const KView& v) {
    if (v.slot_stat) *reinterpret_cast<uint2*>(v.slot_stat) = uint2{v.launch_id, 1u};
}

// The tile pass's pixels by thread, (l << 16 | x), written once by march_kernel: a deferral
// deep in the walk reads its pixel back with one LDS load instead of keeping it live or
// recomputing it from the work and lane orders (two dependent global loads).
__device__ __forceinline__ uint32_t* tile_pixels() {
    __shared__ uint32_t p[64u * kTilesX * kTilesY];
    return p;
}

// CRAWL: fast-forward cluster-skip crawls (the deferred-ray pass); otherwise a
// crawling ray reserves an entry in the launch's deferral list and unwinds.
// kExact (the crawl pass): every walk runs to its end here, and a loop round that
// leaves its state unchanged is detected as a walk that never finishes.  Otherwise
// (the tile pass) a walk past kTileBudget iterations is handed to the crawl pass.
// (Making the cuckoo store's tile pass exact instead -- it has no cluster skips, so
// no crawls, and could do without a crawl pass -- keeps the round-state snapshot live
// through its walk loop: C4 0.085 -> 0.109 ms per frame, profiles/r03/ab_exact_cuckoo.txt.)
template <int STORE, bool CRAWL>
struct ExactWalk { static constexpr bool value = CRAWL; };
// PICK (pick_kernel only): the walk also brings out the grid cell of the probe that read the
// primary hit's colour (PickCell::pv, region-local, as probed).  Every write to it sits under
// `if constexpr (PICK)` and the render and crawl kernels' walkers have no such member, so
// those kernels carry no extra value (their resource usage is unchanged: profiles/pick/).
template <bool PICK> struct PickCell {};
template <> struct PickCell<true> { i3 pv{0, 0, 0}; };
template <int STORE, bool COUNT, bool CRAWL, bool PICK = false>
struct Walker : Ctx<STORE, COUNT, ExactWalk<STORE, CRAWL>::value ? kCrawlBudget : kTileBudget>, PickCell<PICK> {
    using C = Ctx<STORE, COUNT, ExactWalk<STORE, CRAWL>::value ? kCrawlBudget : kTileBudget>;
    static constexpr bool kExact = ExactWalk<STORE, CRAWL>::value;
    static constexpr uint32_t kBudget = C::kBudget;
    using C::s; using C::v; using C::aborted; using C::tick; using C::exists; using C::lookup;
    using C::lighting; using C::normal_from_t; using C::in_region; using C::grid_in_region;
    using C::advance_region; using C::in_scene; using C::region_at; using C::skip_null; using C::bytes;
    __device__ Walker(const KScene& s_, const KView& v_) : C(s_, v_) {}
    // Per-ray reciprocals for the entry clip and each region walk's initial step
    // (div_fast instead of IEEE division): cuckoo C4 -2.5 %, but the VCS walks'
    // kernel runs at its 72-VGPR limit and the longer-lived values cost spills
    // there (C2 +1.6 %, C3 +4 %), so VCS keeps the plain divisions.
    static constexpr bool kFastSetup = STORE == STORE_HASH;
    // VR_LONG_REMAT (the VCS longest-axis tile pass): see primary_regions
#ifndef VR_LONG_REMAT
#define VR_LONG_REMAT 1
#endif
    static constexpr bool kRematDir = VR_LONG_REMAT && STORE == STORE_VCS && !CRAWL;
    // what a deferred crawl must know to be resumed (see the deferral below):
    // bit 1 = the shadow walk is the longest-axis one; the lit colour of the hit
    uint32_t ctx = 0, lit_saved = 0;
    // Crawl pass (VCS): this lane's LDS copy of the cluster-existence bits of region
    // bm_reg (KScene::vcs_cbits, 16 words), or null.  A crawl record's remaining walk
    // -- up to ~280 iterations, mostly cluster skips through C5's empty clusters, each
    // a dependent mask load from MALL/HBM -- then loads a mask word only in present
    // clusters: a skip step reads one LDS word instead.
    uint32_t* lbm = nullptr;
    uint32_t bm_reg = kNone;
    // Crawl pass (VCS) at more records per wave than it has LDS slots (lbm null): the walk
    // loop loads every mask word, but a crawl's closed form (crawl_run) still crosses the
    // faces of absent clusters, reading the region's bits from memory -- the same iterations
    // are fast-forwarded at every width.
    bool mem_bits = false;

    // rayMarchVoxelGrid (Renderer.cuh:260-336) and, SHADOW, shadowRayMarchVoxelGrid (:100-172).
    // The cluster-skip step (:290-306) and the voxel step (:318-331) share one
    // code path: both are o += (min_i (target_i - o_i) / d_i + EPSILON) * d with
    // target = the cluster plane (int, no EPSILON) or ceilf/floorf(o) +- EPSILON;
    // only the voxel step refreshes the t values the hit normal reads (the skip
    // branch's are block-scoped).  One set of IEEE divisions per
    // iteration instead of two divergent ones.  Lighting is applied by the
    // caller after the walk (Hit carries colour, normal and position).
    // EQ (shadow walks only): the direction's components are equal (the
    // default light, normalize(1,1,1), Main.cu:28).  Then every t_i = a_i / d
    // shares one divisor, and correctly rounded division is monotone in the
    // numerator, so min_i RN(a_i / d) = RN(min_i a_i / d) (max_i for d < 0):
    // one division per iteration instead of three, and (t + EPSILON) * d_i is
    // one product.  Bit-identical; shadow walks read no per-axis t values.
    template <bool SHADOW, bool EQ = false>
    __device__ __forceinline__ bool grid_original(f3& o, f3 d, uint32_t reg, i3 cr, Hit& h,
                                                  const uint32_t* rs = nullptr, const Rcp* rc = nullptr) {
        return grid_original_rt(o, d, reg, cr, h, SHADOW, SHADOW && EQ, rs, rc);
    }
    // The same with the shadow flag a per-lane value (fused primary + shadow
    // walk); the template form above constant-folds it.
    // rs (crawl pass only): a deferral record -- resume the walk at its crawl.
    // rc: the ray's reciprocals rcp_setup(d.x), (d.y), (d.z), made once per ray
    // (nullptr: made here).
    // generic: one loop for every sign pattern (the longest-axis walks' rare
    // original-DDA tails: less code and register demand in that kernel)
    // AX, AY, AZ, aw (the tile pass's original shadow walk, see arms): the caller runs inside
    // the arm of the ray's sign pattern -- +1 / -1 per axis, or 2, 2, 2 for all positive with the
    // reciprocals in div_fast's domain; rc and aw are then the ray's.  No dispatch here:
    // the signs, the +-1, +-EPSILON and cluster-offset constants and the planes of the
    // initial step fold at compile time.  0, 0, 0: the signs are read from d in here.
    template <int AX = 0, int AY = 0, int AZ = 0>
    __device__ __forceinline__ bool grid_original_rt(f3& o, f3 d, uint32_t reg, i3 cr, Hit& h, const bool SHADOW,
                                                     const bool EQ, const uint32_t* rs = nullptr,
                                                     const Rcp* rc = nullptr, const bool generic = false,
                                                     const ArmRay* aw = nullptr) {
        constexpr bool kArm = AX != 0;
        static_assert(!kArm || !CRAWL, "sign arms are the tile pass's");
        // the set-up's plane signs (plane_v: 0 = per lane)
        constexpr int BX = AX > 0 ? 1 : AX, BY = AY > 0 ? 1 : AY, BZ = AZ > 0 ? 1 : AZ;
        const bool resume = CRAWL && rs != nullptr;
        VR_DIAG_COUNT(SHADOW ? 9 : 8);                 // grid_original calls
        const bool px = kArm ? AX > 0 : d.x > 0.0f, py = kArm ? AY > 0 : d.y > 0.0f, pz = kArm ? AZ > 0 : d.z > 0.0f;
        // (a positive component is not zero)
        const bool zx = SHADOW && !(kArm && AX > 0) && d.x == 0.0f, zy = SHADOW && !(kArm && AY > 0) && d.y == 0.0f,
                   zz = SHADOW && !(kArm && AZ > 0) && d.z == 0.0f;
        float tX, tY, tZ;
        if (resume) {                             // o is the stepped position of the crawl
            tX = __uint_as_float(rs[11]); tY = __uint_as_float(rs[12]); tZ = __uint_as_float(rs[13]);
        } else if (!CRAWL) {
            // The initial step (Renderer.cuh:269-280; shadow :106-117) with the ray's
            // hoisted reciprocals (or the walk's own, which its loop shares): |n| <= 1 +
            // EPSILON here, so the fast division's domain is the direction's plus
            // |n| >= 2^-90 (see div_fast).
            const bool use_rc = rc && (kFastSetup || SHADOW);
            const Rcp r0x = use_rc ? rc[0] : rcp_setup(d.x), r0y = use_rc ? rc[1] : rcp_setup(d.y),
                      r0z = use_rc ? rc[2] : rcp_setup(d.z);
            const float sx = px ? 1.0f : -1.0f, sy = py ? 1.0f : -1.0f, sz = pz ? 1.0f : -1.0f;
            const float ax = plane_v<BX>(o.x, sx, sx * kEps) - o.x, ay = plane_v<BY>(o.y, sy, sy * kEps) - o.y,
                        az = plane_v<BZ>(o.z, sz, sz * kEps) - o.z;
            // (an arm: aw->nlim is 2^-90 where the three reciprocals are in the domain and no
            // component is a guarded zero, else +inf)
            const bool fast = kArm ? fminf(fabsf(ax), fminf(fabsf(ay), fabsf(az))) >= aw->nlim
                                   : r0x.ok && r0y.ok && r0z.ok && !zx && !zy && !zz &&
                                         fminf(fabsf(ax), fminf(fabsf(ay), fabsf(az))) >= 0x1p-90f;
            tX = div_fast(ax, r0x); tY = div_fast(ay, r0y); tZ = div_fast(az, r0z);
            if (__builtin_expect(__builtin_amdgcn_ballot_w64(!fast) != 0, 0)) {
                VR_DIAG_COUNT(32);                     // initial step: a lane outside div_fast's domain
                tX = fast ? tX : (zx ? kInf : ax / d.x);
                tY = fast ? tY : (zy ? kInf : ay / d.y);
                tZ = fast ? tZ : (zz ? kInf : az / d.z);
            }
            o = add(o, scl(fminf(tX, fminf(tY, tZ)) + kEps, d));
        } else {
            const float nX = px ? ceilf(o.x) + kEps : floorf(o.x) - kEps;
            const float nY = py ? ceilf(o.y) + kEps : floorf(o.y) - kEps;
            const float nZ = pz ? ceilf(o.z) + kEps : floorf(o.z) - kEps;
            tX = zx ? kInf : (nX - o.x) / d.x;
            tY = zy ? kInf : (nY - o.y) / d.y;
            tZ = zz ? kInf : (nZ - o.z) / d.z;
            o = add(o, scl(fminf(tX, fminf(tY, tZ)) + kEps, d));
        }
        uint32_t col = kEmpty;
        if constexpr (STORE == STORE_VCS) {
            // Inside the region every voxel coordinate is in [0, 64): the mask
            // word index is a few bit operations and the lookup needs no
            // range check (Ctx::lookup's general form handles the rest).
            const uint2* mreg = s.vcs_mask + (size_t)reg * 8192u;
            // the region's mask words as a 32-bit byte offset from the scene's (uniform)
            // mask array: the loads take the SGPR-base form (one VGPR, no 64-bit add)
            const uint32_t moff = reg << 16;
            // (crawl pass) the region's cluster-existence bits in LDS: the workgroup's copy of
            // the scene's, or this lane's slot, refilled when the walk enters another region
            const uint32_t* bits = nullptr;
            if constexpr (CRAWL) {
                if (lbm) {
                    if (reg != bm_reg) {
                        const uint4* src = reinterpret_cast<const uint4*>(s.vcs_cbits + (size_t)reg * 16u);
                        const uint4 b0 = src[0], b1 = src[1], b2 = src[2], b3 = src[3];
                        uint4* dst = reinterpret_cast<uint4*>(lbm);
                        dst[0] = b0; dst[1] = b1; dst[2] = b2; dst[3] = b3;
                        bm_reg = reg;
                    }
                    bits = lbm;
                }
            }
            const uint32_t* run_bits = bits;       // crawl_run's
            if constexpr (CRAWL) {
                if (!bits && mem_bits) run_bits = s.vcs_cbits + (size_t)reg * 16u;
            }
            // Straight-line body with one exit: the hit test, the region test of
            // the stepped position and the iteration budget are folded into a
            // single condition; the step of the hit iteration is computed and
            // discarded (the reference breaks before it).  tick() semantics are
            // kept: iteration k of the pixel runs iff k <= kBudget.
            o = add(o, f3{0.0f, 0.0f, 0.0f});      // -0 -> +0 (in_region_bits_nz below)
            if (!this->in_region_bits_nz(o)) return false;
            if (aborted || this->iters >= kBudget) { aborted = true; return false; }
            bool found = false, inside = true, crawl = false;
            // crawl exits (see crawl_steps): from this iteration count on (crawl pass);
            // tile pass: until a deferral failed
            uint32_t crawl_after = 0;
            bool crawl_off = false;
            uint32_t vi = 0;
            int32_t qx = 0, qy = 0, qz = 0;   // crawl pass: voxel of the iteration that exited to crawl
            Blk blk{0u, kNone};
            uint32_t bit = 0;
            bool resume_now = resume;
            for (;;) {
                // Per-walk constants, (re)made here in the crawl pass so they are
                // dead across the crawl code below (the barrier keeps them from
                // being hoisted).
                f3 dl = d;
                if (CRAWL) asm("" : "+v"(dl.x), "+v"(dl.y), "+v"(dl.z));
                // Hoisted reciprocals (div_fast) and +-1 plane signs for the loop
                // (rcp_setup(-d) = -rcp_setup(d) bit for bit: tools/div_proof.hip).
                Rcp rx, ry, rz;
                if (rc && !CRAWL && (kFastSetup || SHADOW)) {
                    rx = EQ ? Rcp{fabsf(dl.x), fabsf(rc[0].r), rc[0].ok} : rc[0];
                    ry = rc[1];
                    rz = rc[2];
                } else {
                    rx = rcp_setup(EQ ? fabsf(dl.x) : dl.x); ry = rcp_setup(dl.y); rz = rcp_setup(dl.z);
                }
                const float gx = px ? 1.0f : -1.0f, gy = py ? 1.0f : -1.0f, gz = pz ? 1.0f : -1.0f;
                const float ex = gx * kEps, ey = gy * kEps, ez = gz * kEps;
                const int32_t cx8 = px ? 8 : 0, cy8 = py ? 8 : 0, cz8 = pz ? 8 : 0;
                // A guarded zero direction component (shadow ray) keeps the lane on the
                // slow branch, which applies the guard: the fast path needs no selects.
                // one compare per iteration: min |n| >= lim (lim = +inf sends the lane
                // to the slow branch every iteration; |n| < 73 inside a region)
                // (an arm: both made once per ray)
                const float nlim0 = kArm ? aw->nlim : 0.0f;
                const bool walk_ok = kArm ? nlim0 < kInf : rx.ok && ry.ok && rz.ok && !zx && !zy && !zz;
                const float nlim = kArm ? nlim0 : (walk_ok ? 0x1p-90f : kInf);
                if (resume_now) {
                    // the deferred crawl: its iteration left an absent cluster (blk) at
                    // voxel q with o stepped; the post-loop test below re-finds the crawl
                    resume_now = false;
                    blk = Blk{0u, kNone};
                    bit = 0;
                    qx = (int32_t)rs[15]; qy = (int32_t)rs[16]; qz = (int32_t)rs[17];
                } else {
                    // The loop, specialised for a wave whose lanes share the signs of the
                    // direction (nearly every primary tile; every shadow walk): the planes
                    // then need no sign multiplications (see plane_v / plane_c8).
                    auto walk = [&](auto SXc, auto SYc, auto SZc) {
                        constexpr int SX = decltype(SXc)::value, SY = decltype(SYc)::value, SZ = decltype(SZc)::value;
                        // All three components positive (every lane of this pass, and every
                        // lane's reciprocals in div_fast's domain: checked before this loop is
                        // chosen): then no numerator is ever tiny or zero -- a voxel plane lies
                        // >= ~EPSILON/2 beyond o, a cluster plane (v & ~7) + 8 > o by >= ulp(64)
                        // -- so the division needs no fallback, and no crawl (t = 0) can occur.
                        // (Sgn<2>: positive, and the caller checked the reciprocals)
                        constexpr bool kPos = SX == 2 && SY == 2 && SZ == 2;
                        // The iteration count as the budget test reads it, biased so that
                        // it reaches bits(64.0f) exactly when iters exceeds kBudget:
                        // one add per iteration.
                        uint32_t ic = this->iters + (0x42800000u - kBudget);
                        // Every lane's direction in div_fast's domain (nearly every walk): then
                        // only a cluster-skip plane can give a numerator outside it -- a voxel
                        // plane (ceilf(o) + EPSILON, floorf(o) - EPSILON) lies >= ~EPSILON/2 from
                        // o -- so the domain check runs only in wave-iterations where some lane
                        // skips (a scalar branch; -2 VALU per iteration without a skip).
                        // (an arm: the ray's, uniform)
                        const bool okw = kArm ? aw->okw : __builtin_amdgcn_ballot_w64(!walk_ok) == 0;
                        VR_DIAG_COUNT((SHADOW ? 4 : 0) + (SX == 0 ? 1 : 0));   // walk entries
                        const float neg_eps = walk_const(-kEps);   // (bit_sel's)
                        for (;;) {
                            VR_DIAG_COUNT((SHADOW ? 6 : 2) + (SX == 0 ? 1 : 0));   // loop iterations
                            // (o is in the region here, so the plain cast is f2i; the mask word's
                            // byte offset is one statement read by the load alone: see Ctx::cell)
                            const int32_t vx = this->cell(o.x), vy = this->cell(o.y), vz = this->cell(o.z);
                            this->count(4);
                            const uint32_t woff = this->template word_offset<3u>((uint32_t)vx, (uint32_t)vy, (uint32_t)vz, moff);
                            [[maybe_unused]] const uint32_t wi = (woff >> 3) & 8191u;   // (crawl pass, COUNT)
                            if constexpr (CRAWL) {
                                // (crawl pass) cluster slot wi >> 4 absent per the LDS bits: no load
                                const bool pres = !bits || ((bits[wi >> 9] >> ((wi >> 4) & 31u)) & 1u);
                                if (COUNT && !pres) ++this->nl;   // counted above, never loaded
                                blk = Blk{0u, kNone};
                                if (pres)
                                    blk = this->mask_at(woff);
                            } else {
                                blk = this->mask_at(woff);
                            }
                            __builtin_amdgcn_sched_barrier(0);   // issue the load before the planes
                            // both candidate planes, computed while the mask word is in
                            // flight and materialised before the wait for it (the second
                            // barrier; the word itself is no operand of the asm, whose results
                            // the next instruction, the compare of blk.y, would then read)
#if VR_UNIFORM_SKIP
                            float vX = plane_v<SX>(o.x, gx, ex), vY = plane_v<SY>(o.y, gy, ey), vZ = plane_v<SZ>(o.z, gz, ez);
                            asm("" : "+v"(vX), "+v"(vY), "+v"(vZ));
                            // (the count's add as asm: loop strength reduction otherwise keeps two
                            // counters; here, so that its reader -- the exit test -- is far from it)
                            asm("v_add_u32 %0, 1, %0" : "+v"(ic));
                            __builtin_amdgcn_sched_barrier(0);
                            const bool skip = absent(blk);
                            float nX = vX, nY = vY, nZ = vZ;
                            const bool any_skip = __builtin_amdgcn_ballot_w64(skip) != 0;
                            if (any_skip) {
                                float cX = (float)((vx & 0x38) + plane_c8<SX>(cx8)), cY = (float)((vy & 0x38) + plane_c8<SY>(cy8)),
                                      cZ = (float)((vz & 0x38) + plane_c8<SZ>(cz8));
                                nX = skip ? cX : vX; nY = skip ? cY : vY; nZ = skip ? cZ : vZ;
                                // (keeps the selects in this block; the values are inputs only:
                                // as results, the step's subtractions would read an asm's)
                                asm volatile("" : : "v"(nX), "v"(nY), "v"(nZ));
                            }
#else
                            float vX = plane_v<SX>(o.x, gx, ex), vY = plane_v<SY>(o.y, gy, ey), vZ = plane_v<SZ>(o.z, gz, ez);
                            // (in the region v < 64, so v & ~7 == v & 0x38, the form word_index shares)
                            float cX = (float)((vx & 0x38) + plane_c8<SX>(cx8)), cY = (float)((vy & 0x38) + plane_c8<SY>(cy8)),
                                  cZ = (float)((vz & 0x38) + plane_c8<SZ>(cz8));
                            asm("" : "+v"(vX), "+v"(vY), "+v"(vZ), "+v"(cX), "+v"(cY), "+v"(cZ), "+v"(blk.x), "+v"(blk.y));
                            asm("v_add_u32 %0, 1, %0" : "+v"(ic));   // (the count: see above)
                            const bool skip = absent(blk);
                            const bool any_skip = __builtin_amdgcn_ballot_w64(skip) != 0;
#endif
                            const bool chk = !kPos && (!okw || any_skip);   // (uniform)
#ifdef VR_DIAG
                            {   // wave-iterations where no active lane / every active lane skips a cluster
                                const uint64_t bs = __builtin_amdgcn_ballot_w64(skip);
                                if (bs == 0) VR_DIAG_COUNT(SHADOW ? 24 : 22);
                                else if (bs == __builtin_amdgcn_read_exec()) VR_DIAG_COUNT(SHADOW ? 25 : 23);
                            }
#endif
                            bit = this->word_bit5c((uint32_t)vy, (uint32_t)vz);
                            // 0 or ~0 (an absent cluster's words have no bits set)
                            const uint32_t fm = (uint32_t)__builtin_amdgcn_sbfe((int32_t)blk.x, bit, 1u);
                            found = fm != 0u;
                            vi = blk.y + __popc(blk.x & ((1u << (bit & 31u)) - 1u));
                            if (COUNT && !skip) this->count_bsearch(mreg + (wi & ~15u), vi, found);
#if !VR_UNIFORM_SKIP
                            const float nX = skip ? cX : vX;
                            const float nY = skip ? cY : vY;
                            const float nZ = skip ? cZ : vZ;
#endif
                            const float ax = nX - o.x, ay = nY - o.y, az = nZ - o.z;
                            float sMin;
                            crawl = false;
                            if (EQ) {
                                // |a_i| / |d| = a_i / d up to the sign of a zero (t = -0 for
                                // a = +0, d < 0), which neither the step nor the crawl test sees
                                const float am = fminf(fabsf(ax), fminf(fabsf(ay), fabsf(az)));
                                sMin = div_fast(am, rx);
                                if (chk) {
                                    const bool bad = !(am >= nlim);
                                    if (__builtin_expect(__builtin_amdgcn_ballot_w64(bad) != 0, 0)) {
                                        VR_DIAG_COUNT(33);     // VCS walk, one divisor: IEEE fallback
                                        sMin = bad ? am / fabsf(d.x) : sMin;
                                        crawl = bad & walk_ok & skip & (sMin == 0.0f) &
                                                (CRAWL ? ic - (0x42800000u - kBudget) >= crawl_after : !crawl_off);
                                        if (CRAWL && crawl) { qx = vx; qy = vy; qz = vz; }
                                    }
                                }
                            } else {
                                float sX = div_fast(ax, rx), sY = div_fast(ay, ry), sZ = div_fast(az, rz);
                                if (chk) {
                                    const bool bad = !(fminf(fabsf(ax), fminf(fabsf(ay), fabsf(az))) >= nlim);
                                    if (__builtin_expect(__builtin_amdgcn_ballot_w64(bad) != 0, 0)) {
                                        VR_DIAG_COUNT(34);     // VCS walk, three divisors: IEEE fallback
                                        sX = bad ? (zx ? kInf : ax / d.x) : sX;
                                        sY = bad ? (zy ? kInf : ay / d.y) : sY;
                                        sZ = bad ? (zz ? kInf : az / d.z) : sZ;
                                        // a skip step with t = 0 (its plane axis has n = 0, so it is
                                        // always on this branch): the ray creeps through an empty cluster
                                        crawl = bad & walk_ok & skip & (fminf(sX, fminf(sY, sZ)) == 0.0f) &
                                                (CRAWL ? ic - (0x42800000u - kBudget) >= crawl_after : !crawl_off);
                                        if (CRAWL && crawl) { qx = vx; qy = vy; qz = vz; }
                                    }
                                }
                                sMin = fminf(sX, fminf(sY, sZ));
                                const bool vox = !skip && !found;        // a voxel step: its t values feed the normal
                                tX = vox ? sX : tX; tY = vox ? sY : tY; tZ = vox ? sZ : tZ;   // (tMin: min of the three, at the use)
                            }
                            // A hit keeps o unstepped: its step length becomes (-EPSILON) + EPSILON
                            // = +0 exactly, and o + (+0 * d) = o (o is never -0, d is finite in here).
                            const float ts = bit_sel(fm, neg_eps, sMin) + kEps;
                            o = EQ ? add(o, f3{ts * d.x, ts * d.x, ts * d.x}) : add(o, scl(ts, d));
                            // One unsigned compare for hit, region exit (in_region_bits_nz of the
                            // stepped position) and the budget (iters >= kBudget; ic counts this
                            // iteration already):
                            const uint32_t ev = max(max(max(max(__float_as_uint(o.x), __float_as_uint(o.y)), __float_as_uint(o.z)),
                                                        ic), fm);
                            if (ev >= 0x42800000u || crawl) break;
                        }
                        this->iters = ic - (0x42800000u - kBudget);
                    };
                    const uint32_t sg = (px ? 1u : 0u) | (py ? 2u : 0u) | (pz ? 4u : 0u);
                    using N = Sgn<-1>;
                    using P = Sgn<1>;
                    if constexpr (kArm) {
                        // the caller's arm: this region's walk of its lanes, no dispatch
                        VR_DIAG_PAT(SHADOW, (AX > 0 ? 1 : 0) | (AY > 0 ? 2 : 0) | (AZ > 0 ? 4 : 0));
                        walk(Sgn<AX>{}, Sgn<AY>{}, Sgn<AZ>{});
                    } else if (CRAWL || generic) {
                        walk(Sgn<0>{}, Sgn<0>{}, Sgn<0>{});
                    } else {
                        // One pass of the loop specialised for each sign pattern present in
                        // the wave (nearly always one; a tile straddling a plane where a
                        // direction component changes sign runs two or more, one after the
                        // other).  A generic, per-lane-sign loop in this kernel needed ~81
                        // VGPRs against the specialised loops' ~72 (7 waves/SIMD).  (An
                        // equal-component shadow direction has pattern 0 or 7.)
                        bool todo = true;
#ifdef VR_DIAG
                        uint32_t pass = 0;
#endif
                        while (todo) {
                            const uint32_t pat = __builtin_amdgcn_readfirstlane(sg);
#ifdef VR_DIAG
                            if (++pass == 2u) VR_DIAG_COUNT(41);   // this wave runs a second pattern pass
#endif
                            if (sg == pat) {
                                todo = false;
                                switch (pat) {
                                case 0: VR_DIAG_PAT(SHADOW, 0); walk(N{}, N{}, N{}); break;
                                case 7:
                                    VR_DIAG_PAT(SHADOW, 7);
                                    if (__builtin_amdgcn_ballot_w64(!walk_ok) == 0) {
                                        walk(Sgn<2>{}, Sgn<2>{}, Sgn<2>{});
                                    } else {
                                        VR_DIAG_COUNT(42);         // a lane's walk_ok failed: P,P,P with checks
                                        walk(P{}, P{}, P{});
                                    }
                                    break;
                                case 1: VR_DIAG_PAT(SHADOW, 1); if (!EQ) walk(P{}, N{}, N{}); break;
                                case 2: VR_DIAG_PAT(SHADOW, 2); if (!EQ) walk(N{}, P{}, N{}); break;
                                case 3: VR_DIAG_PAT(SHADOW, 3); if (!EQ) walk(P{}, P{}, N{}); break;
                                case 4: VR_DIAG_PAT(SHADOW, 4); if (!EQ) walk(N{}, N{}, P{}); break;
                                case 5: VR_DIAG_PAT(SHADOW, 5); if (!EQ) walk(P{}, N{}, P{}); break;
                                default: VR_DIAG_PAT(SHADOW, 6); if (!EQ) walk(N{}, P{}, P{}); break;
                                }
                            }
                        }
                    }
                }
                // Why the lane left, recomputed from values the loop keeps in VGPRs
                // anyway (a flag read after a divergent loop is carried through it as
                // a lane mask, at three scalar ops per flag per iteration; the barrier
                // keeps the compiler from reusing the in-loop flags): a hit leaves o
                // unstepped (inside), and a crawl is the one remaining exit.
                asm("" : "+v"(blk.x), "+v"(blk.y), "+v"(bit), "+v"(o.x), "+v"(o.y), "+v"(o.z), "+v"(this->iters));
                found = !absent(blk) & (__builtin_amdgcn_ubfe(blk.x, bit, 1u) != 0u);
                inside = found || this->in_region_bits_nz(o);
                crawl = !found && inside && this->iters < kBudget;
                if (!crawl || !inside || this->iters >= kBudget) break;
                if constexpr (!CRAWL) {
                    // Defer only a real crawl: an axis on its own skip plane that
                    // EPSILON * d cannot move (it did not: o is the stepped position),
                    // so t = 0 again and again.  A one-off t = 0 step walks on here.
                    // (o on its plane (v & ~7) <=> o / 8 is an integer; o * 0.125 is exact)
                    const bool kx = !px && truncf(o.x * 0.125f) == o.x * 0.125f && o.x + kEps * d.x == o.x;
                    const bool ky = !py && truncf(o.y * 0.125f) == o.y * 0.125f && o.y + kEps * d.y == o.y;
                    const bool kz = !pz && truncf(o.z * 0.125f) == o.z * 0.125f && o.z + kEps * d.z == o.z;
                    // Defer the whole pixel to the crawl pass if a list entry is
                    // free (unwinds like an abort); otherwise walk on plainly.
                    if ((kx || ky || kz) && v.defer) {
                        const uint32_t idx = atomicAdd(v.defer, 1u);
                        deferral_report(v);
                        if (idx < v.defer_cap) {
                            // (the tile pass writes this pixel as 0; the crawl pass,
                            // which runs after it, overwrites it and counts its bytes)
                            uint32_t* r = v.defer + 4 + (size_t)idx * kDeferRecWords;
                            r[0] = tile_pixels()[threadIdx.x];   // (l << 16 | x), from LDS: not kept live through the walk
                            r[1] = (SHADOW ? 1u : 0u) | this->ctx;
                            r[2] = __float_as_uint(o.x); r[3] = __float_as_uint(o.y); r[4] = __float_as_uint(o.z);
                            r[5] = (uint32_t)cr.x; r[6] = (uint32_t)cr.y; r[7] = (uint32_t)cr.z;
                            r[8] = v.launch_id;                         // (the crawl pass takes only its launch's)
                            r[9] = this->iters;
                            r[10] = this->bytes;
                            // (a shadow walk has no normal: its t values are not kept live for this)
                            r[11] = SHADOW ? 0u : __float_as_uint(tX); r[12] = SHADOW ? 0u : __float_as_uint(tY);
                            r[13] = SHADOW ? 0u : __float_as_uint(tZ); r[14] = 0u;   // reserved
                            // (the crawl iteration's voxel q, words 15-17, is recovered from the
                            // stepped position by the crawl pass: see crawl_kernel)
                            r[1] |= v.crawl_rewalk ? 4u : 0u;
                            r[18] = this->lit_saved;
                            // (the flag that the record exists is this sentinel: a bool here would
                            // be carried through every loop as a lane mask -- SGPR spills)
                            this->iters = kDeferredIters;
                            aborted = true;
                            return false;
                        }
                    }
                    if (kx || ky || kz) crawl_off = true;
                } else {
                    // Off the hot loop: fast-forward the identical crawl iterations
                    // exactly, then resume the walk (no region-entry step).
#ifdef VR_CRAWL_PROF
                    const uint32_t n = crawl_run(o, d, qx, qy, qz, px, py, pz, kBudget - this->iters, run_bits, &this->d_trips);
#else
                    const uint32_t n = crawl_run(o, d, qx, qy, qz, px, py, pz, kBudget - this->iters, run_bits);
#endif
                    // none (not a real crawl, or its next step leaves the cluster): a few plain
                    // iterations, then re-arm
                    if (n == 0u) {
                        crawl_after = this->iters + 8u;
                    } else {
                        this->iters += n;
                        this->count_ff(n);
                        inside = this->in_region_bits_nz(o);
                        if (!inside || this->iters >= kBudget) break;
                    }
                }
            }
            if (!found) {
                if (inside) aborted = true;     // the next iteration's tick() would have failed
                return false;
            }
            col = s.vcs_vals[vi];
        } else {
            // Cuckoo store (doesVoxelSpaceExist is always true: no cluster skips).
            // Every iteration looks its voxel's key up (CuckooHashTable::lookupVoxel,
            // CuckooHashTable.cuh:59-76).  A key that is not in the tables -- nearly every
            // probe of a walk -- costs the reference key1 and key2 (8 B) and misses: that is
            // answered by the region's key-presence filter (KScene::ht_filter, one bit per
            // voxel, the VCS mask-word order: a wave's neighbouring rays read neighbouring
            // words), so the loop is one coalesced 4-B load, the voxel step and one exit test.
            // The key that IS present ends the walk: after the loop its two slots are probed
            // as the reference does (key1, val1 on a match, else key2, val2), and the bytes
            // of the table it was found in are counted.  (Round 4 probed both slots of every
            // iteration -- random HBM reads, 2.3x the algorithmic bytes at C4, L2 hit 0.55.)
            o = add(o, f3{0.0f, 0.0f, 0.0f});      // -0 -> +0 (in_region_bits_nz below)
            if (!this->in_region_bits_nz(o)) return false;
            if (aborted || this->iters >= kBudget) { aborted = true; return false; }
            // (an arm: the ray's reciprocals; rcp_setup(|d|) = |rcp_setup(d)|, see the VCS walk)
            const bool arm_rc = kArm && rc;
            const Rcp rx = arm_rc ? (EQ ? Rcp{fabsf(d.x), fabsf(rc[0].r), rc[0].ok} : rc[0]) : rcp_setup(EQ ? fabsf(d.x) : d.x),
                      ry = arm_rc ? rc[1] : rcp_setup(d.y), rz = arm_rc ? rc[2] : rcp_setup(d.z);
            const float gx = px ? 1.0f : -1.0f, gy = py ? 1.0f : -1.0f, gz = pz ? 1.0f : -1.0f;
            const float ex = gx * kEps, ey = gy * kEps, ez = gz * kEps;
            // (an arm: walk_ok, nlim and okw are the ray's, see the VCS walk)
            const float nlim0 = kArm ? aw->nlim : 0.0f;
            const bool walk_ok = kArm ? nlim0 < kInf : rx.ok && ry.ok && rz.ok && !zx && !zy && !zz;
            const float nlim = kArm ? nlim0 : (walk_ok ? 0x1p-90f : kInf);
            // no cluster skips here: with every lane's direction in div_fast's domain no
            // numerator (a voxel plane's, >= ~EPSILON/2 from o) leaves it -- no check at all
            const bool okw = kArm ? aw->okw : __builtin_amdgcn_ballot_w64(!walk_ok) == 0;
            // the region's filter words (64-bit: a cuckoo scene has no region bound, vr_internal.h)
            const uint32_t* freg = s.ht_filter + (size_t)reg * kHashFilterWords;
            uint32_t fw = 0, bit = 0;
            uint32_t ic = this->iters + (0x42800000u - kBudget);   // biased count (see the VCS walk)
            // rayMarchVoxelGrid's voxel step (Renderer.cuh:318-331) from o: its t values, min
            auto voxel_step = [&](float& sX, float& sY, float& sZ) -> float {
                const float ax = plane_v<BX>(o.x, gx, ex) - o.x, ay = plane_v<BY>(o.y, gy, ey) - o.y,
                            az = plane_v<BZ>(o.z, gz, ez) - o.z;
                if (EQ) {                                 // see grid_original
                    const float am = fminf(fabsf(ax), fminf(fabsf(ay), fabsf(az)));
                    float sMin = div_fast(am, rx);
                    if (!okw) {
                        const bool bad = !(am >= nlim);
                        if (__builtin_expect(__builtin_amdgcn_ballot_w64(bad) != 0, 0)) {
                            VR_DIAG_COUNT(35);             // cuckoo walk, one divisor: IEEE fallback
                            sMin = bad ? am / fabsf(d.x) : sMin;
                        }
                    }
                    return sMin;
                }
                sX = div_fast(ax, rx); sY = div_fast(ay, ry); sZ = div_fast(az, rz);
                if (!okw) {
                    const bool bad = !(fminf(fabsf(ax), fminf(fabsf(ay), fabsf(az))) >= nlim);
                    if (__builtin_expect(__builtin_amdgcn_ballot_w64(bad) != 0, 0)) {
                        VR_DIAG_COUNT(36);                 // cuckoo walk, three divisors: IEEE fallback
                        sX = bad ? (zx ? kInf : ax / d.x) : sX;
                        sY = bad ? (zy ? kInf : ay / d.y) : sY;
                        sZ = bad ? (zz ? kInf : az / d.z) : sZ;
                    }
                }
                return fminf(sX, fminf(sY, sZ));
            };
            for (;;) {
                const int32_t vx = f2i(o.x), vy = f2i(o.y), vz = f2i(o.z);
                const uint32_t wi = this->word_index((uint32_t)vx, (uint32_t)vy, (uint32_t)vz);
                fw = freg[wi];
                __builtin_amdgcn_sched_barrier(0);   // issue the load before the step
                // the voxel step while the word loads
                float sX = 0.0f, sY = 0.0f, sZ = 0.0f;
                const float sMin = voxel_step(sX, sY, sZ);
                // key1 + key2 of a key the tables do not hold; the hit's own bytes are
                // settled after the loop (8 or 12)
                this->count(8u);
                bit = this->word_bit5((uint32_t)vy, (uint32_t)vz);
                const uint32_t fm = (uint32_t)__builtin_amdgcn_sbfe((int32_t)fw, bit, 1u);   // 0 or ~0: present
                if (!SHADOW && !EQ) {                     // a non-hit step: its t values feed the normal
                    tX = fm ? tX : sX; tY = fm ? tY : sY; tZ = fm ? tZ : sZ;
                }
                // a hit keeps o unstepped: step length (-EPSILON) + EPSILON = +0 (see the VCS walk)
                const float ts = bit_select(fm, -kEps, sMin) + kEps;
                o = EQ ? add(o, f3{ts * d.x, ts * d.x, ts * d.x}) : add(o, scl(ts, d));
                asm("v_add_u32 %0, 1, %0" : "+v"(ic));      // (see the VCS walk)
                const uint32_t ev = max(max(max(max(__float_as_uint(o.x), __float_as_uint(o.y)), __float_as_uint(o.z)), ic), fm);
                if (ev >= 0x42800000u) break;
            }
            this->iters = ic - (0x42800000u - kBudget);
            // why the lane left (see the VCS walk): recomputed from VGPR values
            asm("" : "+v"(fw), "+v"(bit), "+v"(o.x), "+v"(o.y), "+v"(o.z));
            if (!__builtin_amdgcn_ubfe(fw, bit, 1u)) {
                if (this->in_region_bits_nz(o)) aborted = true;    // budget spent inside the region
                return false;
            }
            // A shadow walk's hit needs no value: the reference's lookup returns the voxel's
            // colour, and a shadow walk only asks whether it is EMPTY_VAL -- which no stored colour
            // is (< 2^24) -- so the set filter bit (the tables' exact key set) already answers
            // it.  The two random table reads (HBM for C4's 400-MB store) are skipped; the COUNT
            // build still makes them, for the bytes the reference reads (8 or 12).
            col = 0u;                              // (a shadow walk's hit: any colour but EMPTY_VAL)
            if (!SHADOW || COUNT) {
                // the hit (o unstepped: the probed voxel): CuckooHashTable::lookupVoxel's two probes
                const uint32_t key = lshl_or(lshl_or((uint32_t)f2i(o.x), 10u, (uint32_t)f2i(o.y)), 10u, (uint32_t)f2i(o.z));
                const uint4 m = s.ht_meta[reg];    // {base, M, prime, offset}
                const uint2* t1 = s.ht_slots + m.x;
                const uint2 e1 = t1[hash1(key, m.w) % m.y];
                const uint2 e2 = t1[m.y + hash2(key, m.z) % m.y];
                const bool m1 = e1.x == key;
                this->count(m1 ? 0u : 4u);         // key1 + val1 (8, counted above), or key1 + key2 + val2
                col = m1 ? e1.y : e2.y;
            }
        }
        if (col == kEmpty) return false;
        if (!SHADOW) {
            h.col = col;
            // tMin is always min(tX, tY, tZ) of the same step: recomputed here
            // instead of carried through the loop
            h.nc = normal_from_t(tX, tY, tZ, fminf(tX, fminf(tY, tZ)), d);
            h.so = o;
            h.region = cr;
            h.longest = false;
            // (a hit keeps o unstepped: the probed voxel)
            if constexpr (PICK) this->pv = i3{f2i(o.x), f2i(o.y), f2i(o.z)};
        }
        return true;
    }

    // rayMarchVoxelGridLongestAxis (Renderer.cuh:760-915) / shadowRayMarchVoxelGridLongestAxis
    // (:495-631) with performVoxelSpaceJump (:696-751) / performShadowVoxelSpaceJump (:441-492),
    // as a convergent state machine: every loop iteration makes exactly ONE probe
    // (existence check, lookup if present) for every lane, whatever it is doing --
    //   main  : the next axis step of the current iteration of the reference loop
    //           (M/S in crossing order, then L; g[axis] += ad[axis] first), or
    //   jump  : performVoxelSpaceJump's `while (!exists(g))` probes (the first one
    //           re-checks the step's own voxel, as the reference does) and cluster skips,
    // then advances that lane's state.  Same probes, ticks and bytes, in the same
    // order, as the nested reference loops; no per-case code copies, no divergent
    // nesting.  The tail falls back to the original DDA (Renderer.cuh:912).
    template <bool SHADOW>
    __device__ __forceinline__ bool grid_longest(f3& oo, f3 od, uint32_t reg, i3 cr, Hit& h) {
        uint32_t L, M, S;
        // Ray::convertRayToLongestAxisDirection (Ray.cuh:19-71)
        float ax = fabsf(od.x), ay = fabsf(od.y), az = fabsf(od.z), k;
        if (ax > ay && ax > az) {
            L = 0; M = ay > az ? 1 : 2; S = ay > az ? 2 : 1; k = 1.0f / ax;
        } else if (ay > az) {
            L = 1; M = ax > az ? 0 : 2; S = ax > az ? 2 : 0; k = 1.0f / ay;
        } else {
            L = 2; M = ax > ay ? 0 : 1; S = ax > ay ? 1 : 0; k = 1.0f / az;
        }
        const f3 ds = scl(k, od);
        f3 old_o = oo;
        i3 g{f2i(oo.x), f2i(oo.y), f2i(oo.z)};
        i3 ad{0, 0, 0};
        const int32_t adL = comp(od, L) < 0.0f ? -1 : 1;
        seti(ad, L, adL);
        f3 ray_o;
        {
            const float gL = (float)geti(g, L), oL = comp(oo, L);
            const float t = adL > 0 ? (gL + kEps + 1.0f - oL) / (float)adL : (gL - kEps - oL) / (float)adL;
            ray_o = add(old_o, scl(t, ds));
        }
        seti(ad, M, f2i(comp(ray_o, M)) - geti(g, M));
        seti(ad, S, f2i(comp(ray_o, S)) - geti(g, S));
        const bool mid_floor = comp(ds, M) < 0.0f;   // decimalToIntFunc (:784)
        float tX = 0.0f, tY = 0.0f, tZ = 0.0f, tMin = 0.0f;   // the jump's last skip (hit normal)
        uint32_t seq = 0, rem = 0;                   // pending axis steps of this iteration (2 bits each)
        bool jumping = false;

        // Top of the reference's `while (isInGrid(grid + diff))` loop: false = loop over
        // (fall back to the original DDA); aborted = budget exhausted.
        auto begin_iter = [&]() -> bool {
            if (!grid_in_region(g.x + ad.x, g.y + ad.y, g.z + ad.z)) return false;
            if (!tick()) return false;
            const int32_t adM = geti(ad, M), adS = geti(ad, S);
            if (adS != 0 && adM != 0) {
                const float om = comp(old_o, M);
                const float t1 = ((mid_floor ? floorf(om) : ceilf(om)) - om) / comp(ds, M);
                const float sp = comp(old_o, S) + comp(ds, S) * t1;
                const int32_t sd = f2i(floorf(sp)) - geti(g, S);
                const uint32_t a0 = sd != 0 ? S : M, a1 = sd != 0 ? M : S;
                seq = a0 | (a1 << 2) | (L << 4);
                rem = 3;
            } else if (adM != 0) {
                seq = M | (L << 2);
                rem = 2;
            } else if (adS != 0) {
                seq = S | (L << 2);
                rem = 2;
            } else {
                seq = L;
                rem = 1;
            }
            return true;
        };

        bool tail = !begin_iter();
        if (aborted) return false;
        while (!tail) {
            const uint32_t axis = seq & 3u;
            i3 pg = g;
            if (!jumping) seti(pg, axis, geti(g, axis) + geti(ad, axis));
            const Blk blk = exists(reg, pg.x, pg.y, pg.z);
            const bool present = !absent(blk);
            const uint32_t col = present ? lookup(reg, blk, pg.x, pg.y, pg.z) : kEmpty;
            g = pg;
            if (col != kEmpty) {
                if (!SHADOW) {
                    h.col = col;
                    h.region = cr;
                    h.longest = true;
                    if constexpr (PICK) this->pv = pg;
                    if (jumping) {                   // performVoxelSpaceJump's hit
                        h.nc = normal_from_t(tX, tY, tZ, tMin, ds);
                        h.so = old_o;
                    } else {                         // an axis step's hit
                        h.nc = this->ncode(axis, copysignf(1.0f, -comp(ds, axis)));
                        if (axis == L) {
                            h.so = ray_o;
                        } else {                     // getLocalHitLocation (Renderer.cuh:753-758)
                            const float o = comp(old_o, axis), dd = comp(ds, axis);
                            const float t = dd > 0.0f ? (ceilf(o) - o) / dd : (floorf(o) - o) / dd;
                            h.so = add(old_o, scl(t, ds));
                        }
                    }
                }
                return true;
            }
            if (!jumping) {
                if (!present) { jumping = true; continue; }   // performVoxelSpaceJump (re-probes g)
                seq >>= 2;
                if (--rem != 0u) continue;
                old_o = ray_o;                       // end of the iteration (:903-906)
                ray_o = add(ray_o, ds);
                seti(ad, M, f2i(comp(ray_o, M)) - geti(g, M));
                seti(ad, S, f2i(comp(ray_o, S)) - geti(g, S));
                tail = !begin_iter();
                if (aborted) return false;
                continue;
            }
            if (!present) {                          // the jump's cluster skip
                if (!tick()) return false;
                const int32_t nx = ds.x > 0.0f ? ((g.x / 8) + 1) * 8 : (g.x / 8) * 8;
                const int32_t ny = ds.y > 0.0f ? ((g.y / 8) + 1) * 8 : (g.y / 8) * 8;
                const int32_t nz = ds.z > 0.0f ? ((g.z / 8) + 1) * 8 : (g.z / 8) * 8;
                tX = ((float)nx - old_o.x) / ds.x;
                tY = ((float)ny - old_o.y) / ds.y;
                tZ = ((float)nz - old_o.z) / ds.z;
                tMin = fminf(tX, fminf(tY, tZ)) + kEps;
                old_o = add(old_o, scl(tMin, ds));
                g = i3{f2i(floorf(old_o.x)), f2i(floorf(old_o.y)), f2i(floorf(old_o.z))};
                if (!grid_in_region(g.x, g.y, g.z)) {
                    oo = old_o;
                    return false;
                }
                continue;
            }
            // the jump landed in an existing cluster without a hit: CONTINUE_VAL
            const float oL = comp(old_o, L), dL = comp(ds, L);
            const float tNext = dL > 0.0f ? (ceilf(oL) - oL) / dL : (floorf(oL) - oL) / dL;
            ray_o = add(old_o, scl(tNext + kEps, ds));
            seti(ad, M, f2i(comp(ray_o, M)) - geti(g, M));
            seti(ad, S, f2i(comp(ray_o, S)) - geti(g, S));
            jumping = false;
            tail = !begin_iter();
            if (aborted) return false;
        }
        oo = old_o;     // Renderer.cuh:912 (direction of originalRay kept)
        return grid_original<SHADOW>(oo, od, reg, cr, h);
    }

    // The VCS longest-axis walk with ONE reference loop iteration per loop
    // iteration (rayMarchVoxelGridLongestAxis, Renderer.cuh:760-915; shadow twin
    // :495-631; performVoxelSpaceJump :696-751 / :441-492), specialised on the
    // ray's axis order: L, M, S (longest, middle, shortest) are compile-time, so
    // the walk state lives in (L, M, S) registers and no axis is selected at run
    // time (a wave runs one pass per order its lanes hold; shadow rays share one).
    // A lane is either
    //   main : one whole iteration of the reference's while loop -- its probes
    //          are known at its top: slot A (the first crossing, M or S), slot B
    //          (both crossings) and slot C (g + ad, the L step); their three mask
    //          words are loaded together and evaluated in order; the first absent
    //          cluster starts a jump, the first stored voxel is the hit, or
    //   jump : one cluster skip of performVoxelSpaceJump and the probe of the
    //          cell it lands in (slot C; the jump's first existence test re-reads
    //          the probe that started it, known absent: counted, not loaded).
    // Probes, ticks and counted bytes are the reference's, in its order; the
    // later probes of an iteration that stops early are loaded but not counted.
    // Returns the hit; `tail` = the loop ended in the region (the caller runs
    // the original DDA from oo, Renderer.cuh:912-914, once for every order).
    template <int A>
    __device__ __forceinline__ static float ax3(f3 v) { return A == 0 ? v.x : (A == 1 ? v.y : v.z); }
    // ds: the longest-axis direction k * d (Ray.cuh:19-71, made by the caller);
    // cls: its sign classes, the same for every lane of the pass (an SGPR): bit 2a
    // = ds_a > 0, bit 2a+1 = ds_a < 0 (a zero or NaN component is neither), so every
    // direction-sign choice of the walk -- axisDiff[L], decimalToIntFunc, the jump's
    // cluster planes, tNext's ceil/floor -- is a scalar select, not a per-lane mask.
    // UNIT (shadow walks of a light whose ds is (+-1, +-1, +-1) exactly, e.g. the
    // reference's normalize(1,1,1), Main.cu:28): every division by ds_a is exact
    // negation or identity, so it is one multiply (x / +-1 == x * +-1 for every x).
    template <bool SHADOW, bool UNIT, int PL, int PM, int PS>
    __device__ __forceinline__ bool walk_longest_vcs(f3& oo, const f3 ds, const uint32_t cls, uint32_t reg,
                                                     bool& tail, uint32_t& hcol, uint32_t& hcode) {
        const float dL = ax3<PL>(ds), dM = ax3<PM>(ds), dS = ax3<PS>(ds);
        auto dv = [](float n, float d) { return UNIT ? n * d : n / d; };
        // (IEEE divisions here: div_fast with reciprocals made at each use, pinned so they
        // are never loop-carried, measured slower -- C3 0.2264 -> 0.2358 ms per frame,
        // profiles/r04/ab_lfd_rolled.txt -- as every hoisted-reciprocal variant before it)
        auto dv3 = [&](float n0, float d0, float n1, float d1, float n2, float d2, float& q0, float& q1, float& q2) {
            q0 = dv(n0, d0); q1 = dv(n1, d1); q2 = dv(n2, d2);
        };
        auto dv1 = [&](float n, float d) { return dv(n, d); };
        const bool posL = (cls >> (2 * PL)) & 1u, posM = (cls >> (2 * PM)) & 1u, posS = (cls >> (2 * PS)) & 1u;
        const bool negL = (cls >> (2 * PL + 1)) & 1u, negM = (cls >> (2 * PM + 1)) & 1u;
        const int32_t offL = posL ? 8 : 0, offM = posM ? 8 : 0, offS = posS ? 8 : 0;
        // walk frame <-> grid axes (x, y, z): constant indices, registers only
        auto xyz = [](auto l, auto m, auto s) {
            struct { decltype(l) c[3]; } r;
            r.c[PL] = l; r.c[PM] = m; r.c[PS] = s;
            return r;
        };
        auto to_f3 = [&](float l, float m, float s) {
            const auto c = xyz(l, m, s);
            return mk(c.c[0], c.c[1], c.c[2]);
        };
        auto to_i3 = [&](int32_t l, int32_t m, int32_t s) {
            const auto c = xyz(l, m, s);
            return i3{c.c[0], c.c[1], c.c[2]};
        };
        auto word = [&](int32_t l, int32_t m, int32_t s) {
            const auto c = xyz((uint32_t)l & 63u, (uint32_t)m & 63u, (uint32_t)s & 63u);
            return this->word_index(c.c[0], c.c[1], c.c[2]);
        };
        auto bit5 = [&](int32_t l, int32_t m, int32_t s) {
            const auto c = xyz((uint32_t)l, (uint32_t)m, (uint32_t)s);
            return this->word_bit5(c.c[1], c.c[2]) & 31u;
        };
        float oL = ax3<PL>(oo), oM = ax3<PM>(oo), oS = ax3<PS>(oo);      // oldRay origin
        int32_t gL = f2i(oL), gM = f2i(oM), gS = f2i(oS);                 // gridValues
        // axisDiff[L] (d_L < 0 <=> ds_L < 0: k > 0, or k = inf with d = 0, or NaN)
        const int32_t aL = negL ? -1 : 1;
        float rL, rM, rS;                                                 // ray origin
        {
            // x / (float)aL with aL = +-1 is exactly x * aL
            const float t = aL > 0 ? ((float)gL + kEps + 1.0f - oL) * (float)aL : ((float)gL - kEps - oL) * (float)aL;
            rL = oL + t * dL; rM = oM + t * dM; rS = oS + t * dS;
        }
        int32_t aM = f2i(rM) - gM, aS = f2i(rS) - gS;
        const bool mid_floor = negM;                                      // decimalToIntFunc (:784)
        // (IEEE divisions: hoisted reciprocals (div_fast) measured slower here, C3
        // 0.385 -> 0.413 ms -- three more VGPRs live through the loop)
        const uint32_t moff = reg << 16;              // SGPR-base loads (see grid_original_rt)
        auto mload = [&](uint32_t w) {
            return *reinterpret_cast<const uint2*>(reinterpret_cast<const char*>(s.vcs_mask) + (moff | (w << 3)));
        };
        uint32_t nj = 0;                  // the jump's last skip: getNormalFromTValues' axis (x, y, z)
        bool jumping = false;
        uint32_t stop = 3u, col = 0;
        bool mfirst = false;
        // One exit per iteration (each extra exit of a divergent loop costs lane-mask
        // bookkeeping on every iteration): a lane that must leave computes the rest
        // of the iteration on stale values and leaves at its end, with the reason
        // kOver: past the budget; kCrawl (tile pass): a cluster skip with t = 0 -- a jump
        // crawl, 10^4..10^6 iterations in the reference: the crawl pass walks the pixel
        enum : uint32_t { kGo = 0, kHit = 1, kLeft = 2, kOver = 3, kTail = 4, kCrawl = 5 };
        uint32_t why = kGo, it = this->iters;
        VR_DIAG_COUNT(SHADOW ? 19 : 17);               // longest-axis walks
        for (;;) {
            VR_DIAG_COUNT(SHADOW ? 20 : 18);           // longest-axis loop iterations
            VR_DIAG_COUNT_IF(jumping, 21);             // ... with a jumping lane
            // ---- this iteration's probe slots (A.L = B.L = gL)
            int32_t AM, AS, CL, CM, CS;
            bool vA = false, vB = false;
            mfirst = false;
            uint32_t ex;
            if (!jumping) {
                CL = gL + aL; CM = gM + aM; CS = gS + aS;
                // the loop condition (else the original-DDA tail), then tick()
                const bool out = !grid_in_region(CL, CM, CS);
                it += out ? 0u : 1u;
                ex = out ? kTail : (it > kBudget ? kOver : kGo);
                const bool hasM = aM != 0, hasS = aS != 0;
                bool sfirst = false;
                if (hasM && hasS) {
                    const float t1 = dv1((mid_floor ? floorf(oM) : ceilf(oM)) - oM, dM);
                    const float sp = oS + dS * t1;
                    sfirst = f2i(floorf(sp)) - gS != 0;
                }
                vA = hasM || hasS;
                vB = hasM && hasS;
                mfirst = hasM && !sfirst;
                AM = mfirst ? CM : gM;
                AS = mfirst ? gS : CS;
            } else {
                ++it;                                // tick()
                ex = it > kBudget ? kOver : kGo;
                // performVoxelSpaceJump's cluster skip (:707-725), integer planes from g:
                // d > 0 ? ((g / 8) + 1) * 8 : (g / 8) * 8.  (g / 8) * 8 is g & ~7 for g >= 0; the
                // C division form below is for a wave holding a negative cell, and no finite
                // input gives one (counter 37 stays 0; tests/cover_run.py UNREACHABLE):
                //  - a jump goes on from the cell it landed in only if that cell is in the region
                //    (else kLeft ends the walk above), so a negative g would have to be the cell of
                //    the probe that started the jump: slot A, B or C;
                //  - a slot's coordinates are g's or C's = g + a.  C is in the region (else kTail
                //    ended the loop), so a negative coordinate would have to be g's own, and g is
                //    a slot or a landing cell of an earlier iteration -- in the region by the same
                //    argument -- or the walk's first cell f2i(o);
                //  - the walk starts at o = so - 64 * floor(so / 64) >= 0 (primary, advance_region:
                //    the same form after a region is left), or, a shadow walk, at the primary hit's
                //    location, on a face of a voxel of the region: o > -1 on every axis, and f2i
                //    truncates towards zero, so the first cell is >= 0.  (It can be 64,
                //    from o = 64.0 exactly: the probes outside the region that the alias fixture
                //    reaches, counter 38, are all on that side.)
                // Tried on the CPU: tests/test_edge_cases.py::test_no_jump_starts_in_a_negative_cell.
                int32_t bL = gL & ~7, bM = gM & ~7, bS = gS & ~7;
                if (__builtin_expect(__builtin_amdgcn_ballot_w64((gL | gM | gS) < 0) != 0, 0)) {
                    VR_DIAG_COUNT(37);                 // a jumping lane stands in a negative cell
                    bL = (gL / 8) * 8; bM = (gM / 8) * 8; bS = (gS / 8) * 8;
                }
                const int32_t nL = bL + offL, nM = bM + offM, nS = bS + offS;
                float jL, jM, jS;
                dv3((float)nL - oL, dL, (float)nM - oM, dM, (float)nS - oS, dS, jL, jM, jS);
                const auto t = xyz(jL, jM, jS);
                const float tm0 = fminf(t.c[0], fminf(t.c[1], t.c[2]));
                const float tMin = tm0 + kEps;
                nj = t.c[0] == tMin ? 0u : (t.c[1] == tMin ? 1u : 2u);
                const float pL = oL, pM = oM, pS = oS;
                const int32_t qL = gL, qM = gM, qS = gS;
                oL = oL + tMin * dL; oM = oM + tMin * dM; oS = oS + tMin * dS;
                gL = f2i(floorf(oL)); gM = f2i(floorf(oM)); gS = f2i(floorf(oS));
                if (ex == kGo && !grid_in_region(gL, gM, gS)) ex = kLeft;   // left the region: no tail
                // t = 0: the ray stood on a cluster plane.  When EPSILON * d cannot move it
                // off (the axis is still on the plane after the step) every further skip in
                // this cluster is the same: a crawl, for the crawl pass.  A one-off walks on.
                // (The t = 0 axis is M or S: |d_L| ~ 1, so EPSILON * d_L always moves L.)
                if (!CRAWL && ex == kGo && tm0 == 0.0f && (oM == pM || oS == pS)) ex = kCrawl;
                if constexpr (CRAWL) {
                    if (ex == kGo) {
                        if (this->same_f(oL, pL) && this->same_f(oM, pM) && this->same_f(oS, pS) && gL == qL &&
                            gM == qM && gS == qS) {
                            // the skip changed nothing (a NaN position): the jump loop never ends
                            ex = kOver;
                        } else if (tm0 == 0.0f) {
                            // A jump crawl: an axis pinned on its cluster plane that EPSILON * d
                            // cannot move, so every skip in this cluster is o += RN(EPSILON * d)
                            // (tMin = 0 + EPSILON) -- the same recurrence as the original walk's
                            // crawl: fast-forward it exactly (ticks and existence reads credited;
                            // the final position stays in the cluster, so the next skip -- whose t
                            // values a hit's normal reads -- is a plain one).
                            f3 on = to_f3(oL, oM, oS);
                            const f3 dd = to_f3(dL, dM, dS);
                            const i3 q = to_i3(qL, qM, qS);
                            const uint32_t n = crawl_run(on, dd, q.x, q.y, q.z, dd.x > 0.0f, dd.y > 0.0f, dd.z > 0.0f,
                                                         kBudget - it, nullptr
#ifdef VR_CRAWL_PROF
                                                         , &this->d_trips
#endif
                                                         );
                            if (n != 0u) {
                                oL = ax3<PL>(on); oM = ax3<PM>(on); oS = ax3<PS>(on);
                                gL = f2i(floorf(oL)); gM = f2i(floorf(oM)); gS = f2i(floorf(oS));
                                it += n;
                                this->count_ff(n);
                            }
                        }
                    }
                }
                CL = gL; CM = gM; CS = gS;
                AM = gM; AS = gS;
            }
            // ---- the mask words of all slots, requested together
            const uint32_t wA = word(gL, AM, AS), wB = word(gL, CM, CS), wC = word(CL, CM, CS);
            const Blk bA = mload(wA), bB = mload(wB), bC = mload(wC);
            // ---- evaluate the slots in the reference's order (A, B, C)
            const uint32_t iA = bit5(gL, AM, AS), iB = bit5(gL, CM, CS), iC = bit5(CL, CM, CS);
            const bool fA = (bA.x >> iA) & 1u, fB = (bB.x >> iB) & 1u, fC = (bC.x >> iC) & 1u;
            const bool eA = vA && (absent(bA) || fA), eB = vB && (absent(bB) || fB);
            stop = eA ? 0u : (eB ? 1u : ((absent(bC) || fC) ? 2u : 3u));
            bool hit = eA ? fA : (eB ? fB : fC);
            // the value index of the stopping slot only
            const uint32_t sx = eA ? bA.x : (eB ? bB.x : bC.x), sy = eA ? bA.y : (eB ? bB.y : bC.y);
            const uint32_t si = eA ? iA : (eB ? iB : iC);
            col = sy + __popc(sx & ((1u << si) - 1u));
            // huge grid coordinates (A or B outside the region; C is inside): the
            // general (aliasing) form, rare
            const bool inr = ex != kGo || !vA || ((((uint32_t)gL | (uint32_t)AM | (uint32_t)AS) < 64u) &&
                                                  (!vB || (((uint32_t)gL | (uint32_t)CM | (uint32_t)CS) < 64u)));
            if (COUNT && inr && ex == kGo) {
                const i3 P[3] = {to_i3(gL, AM, AS), to_i3(gL, CM, CS), to_i3(CL, CM, CS)};
                const Blk B[3] = {bA, bB, bC};
                const uint32_t W[3] = {wA, wB, wC};
                const bool V[3] = {vA, vB, true};
#pragma unroll
                for (uint32_t i = 0; i < 3u; ++i) {
                    if (!V[i] || i > stop) continue;
                    this->count(4);                   // doesVoxelSpaceExist
                    if (absent(B[i])) continue;
                    const uint32_t bit = this->in_cluster(P[i].x, P[i].y, P[i].z) & 31u;
                    this->count_bsearch(s.vcs_mask + (size_t)reg * 8192u + (W[i] & ~15u),
                                        B[i].y + __popc(B[i].x & ((1u << bit) - 1u)), (B[i].x >> bit) & 1u);
                }
            }
            if (__builtin_expect(__builtin_amdgcn_ballot_w64(!inr) != 0, 0)) {
                VR_DIAG_COUNT(38);                     // a probe slot outside the region: the aliasing form
                if (!inr) {
                    stop = 3u; hit = false; col = kEmpty;
                    const i3 P[3] = {to_i3(gL, AM, AS), to_i3(gL, CM, CS), to_i3(CL, CM, CS)};
                    const bool V[3] = {vA, vB, true};
#pragma unroll
                    for (uint32_t i = 0; i < 3u; ++i) {
                        if (!V[i] || stop != 3u) continue;
                        this->count(4);               // doesVoxelSpaceExist
                        const Blk b = i == 2u ? bC : this->mask_word(reg, P[i].x, P[i].y, P[i].z);
                        if (absent(b)) { stop = i; continue; }
                        if (((uint32_t)P[i].x | (uint32_t)P[i].y | (uint32_t)P[i].z) < 64u) {
                            const uint32_t bit = this->in_cluster(P[i].x, P[i].y, P[i].z) & 31u;
                            const bool f = (b.x >> bit) & 1u;
                            const uint32_t vi = b.y + __popc(b.x & ((1u << bit) - 1u));
                            if (COUNT) this->count_bsearch(this->masks(reg, this->cluster_id(P[i].x, P[i].y, P[i].z)), vi, f);
                            if (f) { stop = i; hit = true; col = vi; }
                        } else {
                            const uint32_t c = this->lookup_aliased(reg, P[i].x, P[i].y, P[i].z);
                            if (c != kEmpty) { stop = i; hit = true; col = c | 0x80000000u; }
                        }
                    }
                }
            }
            if (ex != kGo || hit) {
                why = ex != kGo ? ex : kHit;
                if constexpr (PICK && !SHADOW) {     // the stopping slot's cell (A, B or C)
                    if (why == kHit)
                        this->pv = stop == 0u ? to_i3(gL, AM, AS) : (stop == 1u ? to_i3(gL, CM, CS) : to_i3(CL, CM, CS));
                }
                break;
            }
            if (jumping && stop == 3u) {
                // landed in an existing cluster without a hit: CONTINUE_VAL (:740-750)
                const float tNext = dv1((posL ? ceilf(oL) : floorf(oL)) - oL, dL);
                rL = oL + (tNext + kEps) * dL; rM = oM + (tNext + kEps) * dM; rS = oS + (tNext + kEps) * dS;
            }
            if (!jumping) {
                if (stop != 3u) {                    // an absent cluster: performVoxelSpaceJump
                    this->count(4);                  // its first existence test (this same cell)
                } else {                             // end of the iteration (:903-906)
                    oL = rL; oM = rM; oS = rS;
                    rL = rL + dL; rM = rM + dM; rS = rS + dS;
                }
                // g = the stopping slot (A, B or C), C at the end of the iteration
                gL = stop == 3u || stop == 2u ? CL : gL;
                gM = stop == 0u ? AM : CM;
                gS = stop == 0u ? AS : CS;
            }
            aM = f2i(rM) - gM;                       // (recomputed from unchanged values: same)
            aS = f2i(rS) - gS;
            jumping = stop != 3u;                    // jump on / start a jump; CONTINUE_VAL ends one
        }
        this->iters = it;
        if (why == kOver || why == kCrawl) {   // (tile pass: shade hands the pixel to the crawl pass)
            aborted = true;
            return false;
        }
        if (why == kHit) {
            // the hit as {colour, normal code, location in oo} from the loop's final
            // state: the caller makes the Hit after the original-DDA tail
            if (!SHADOW) {
                hcol = (col & 0x80000000u) ? (col & 0x7FFFFFFFu) : s.vcs_vals[col];
                // normal: axis a (x, y, z) with copysignf(1, -ds[a]): code = a | sign(ds[a]) << 2
                auto code = [](uint32_t a, float d) { return a | ((__float_as_uint(d) >> 31) << 2); };
                if (jumping) {                       // performVoxelSpaceJump's hit (getNormalFromTValues)
                    const auto d = xyz(dL, dM, dS);
                    hcode = code(nj, nj == 0u ? d.c[0] : (nj == 1u ? d.c[1] : d.c[2]));
                    oo = to_f3(oL, oM, oS);
                } else if (stop == 2u) {             // the L step's hit
                    hcode = code(PL, dL);
                    oo = to_f3(rL, rM, rS);
                } else {                             // a crossing's hit: getLocalHitLocation (:753-758)
                    const bool onM = (stop == 0u) == mfirst;
                    const float o = onM ? oM : oS, dd = onM ? dM : dS;
                    hcode = onM ? code(PM, dM) : code(PS, dS);
                    const float t = dd > 0.0f ? (ceilf(o) - o) / dd : (floorf(o) - o) / dd;
                    oo = to_f3(oL + t * dL, oM + t * dM, oS + t * dS);
                }
            }
            return true;
        }
        oo = to_f3(oL, oM, oS);     // Renderer.cuh:912 (direction of originalRay kept)
        tail = why == kTail;
        return false;
    }
    template <bool SHADOW>
    __device__ __forceinline__ bool grid_longest_vcs(f3& oo, f3 od, uint32_t reg, i3 cr, Hit& h) {
        bool hit = false, tail = false;
        uint32_t hcol = 0, hcode = 0;
        if (SHADOW) {
            // the light: its axis order, longest-axis direction and sign classes are
            // made on the host (kernel arguments: SGPRs), one pass
            f3 ds = ld3(v.Lw);
            // (held in VGPRs, though uniform: as SGPRs the direction and everything made from
            // it -- sign classes, plane offsets, the divisions' operands -- overflowed the
            // SGPR file, and the shadow loops restored spilled SGPRs with 16-22 v_readlane per
            // iteration; as VGPRs, 2-6: C3 per frame in flight 0.1888 -> 0.1863 ms, first
            // render 0.2815 -> 0.2758, profiles/r06/ab/ab_C3_vdir.txt)
            asm volatile("" : "+v"(ds.x), "+v"(ds.y), "+v"(ds.z));
            if (v.L_unit) {
                hit = walk_longest_vcs<SHADOW, true, 2, 1, 0>(oo, ds, v.L_cls, reg, tail, hcol, hcode);
            } else {
                switch (v.L_order) {
                    case 0: hit = walk_longest_vcs<SHADOW, false, 0, 1, 2>(oo, ds, v.L_cls, reg, tail, hcol, hcode); break;
                    case 1: hit = walk_longest_vcs<SHADOW, false, 0, 2, 1>(oo, ds, v.L_cls, reg, tail, hcol, hcode); break;
                    case 2: hit = walk_longest_vcs<SHADOW, false, 1, 0, 2>(oo, ds, v.L_cls, reg, tail, hcol, hcode); break;
                    case 3: hit = walk_longest_vcs<SHADOW, false, 1, 2, 0>(oo, ds, v.L_cls, reg, tail, hcol, hcode); break;
                    case 4: hit = walk_longest_vcs<SHADOW, false, 2, 0, 1>(oo, ds, v.L_cls, reg, tail, hcol, hcode); break;
                    default: hit = walk_longest_vcs<SHADOW, false, 2, 1, 0>(oo, ds, v.L_cls, reg, tail, hcol, hcode); break;
                }
            }
        } else {
            // the axis order of convertRayToLongestAxisDirection (Ray.cuh:19-71) and
            // the longest-axis direction k * d, k = 1 / |d_L|
            const float ax = fabsf(od.x), ay = fabsf(od.y), az = fabsf(od.z);
            const uint32_t order =
                (ax > ay && ax > az) ? (ay > az ? 0u : 1u) : (ay > az ? (ax > az ? 2u : 3u) : (ax > ay ? 4u : 5u));
            const float k = 1.0f / (order < 2u ? ax : (order < 4u ? ay : az));
            const f3 ds = scl(k, od);
            const uint32_t cls = (uint32_t)(ds.x > 0.0f) | (uint32_t)(ds.x < 0.0f) << 1 | (uint32_t)(ds.y > 0.0f) << 2 |
                                 (uint32_t)(ds.y < 0.0f) << 3 | (uint32_t)(ds.z > 0.0f) << 4 | (uint32_t)(ds.z < 0.0f) << 5;
            const uint32_t key = order | cls << 3;
            bool todo = true;
            while (todo) {                            // one pass per (order, signs) present in the wave
                const uint32_t pat = __builtin_amdgcn_readfirstlane(key);
                if (key == pat) {
                    todo = false;
                    const uint32_t pc = pat >> 3;
                    switch (pat & 7u) {
                        case 0: hit = walk_longest_vcs<SHADOW, false, 0, 1, 2>(oo, ds, pc, reg, tail, hcol, hcode); break;
                        case 1: hit = walk_longest_vcs<SHADOW, false, 0, 2, 1>(oo, ds, pc, reg, tail, hcol, hcode); break;
                        case 2: hit = walk_longest_vcs<SHADOW, false, 1, 0, 2>(oo, ds, pc, reg, tail, hcol, hcode); break;
                        case 3: hit = walk_longest_vcs<SHADOW, false, 1, 2, 0>(oo, ds, pc, reg, tail, hcol, hcode); break;
                        case 4: hit = walk_longest_vcs<SHADOW, false, 2, 0, 1>(oo, ds, pc, reg, tail, hcol, hcode); break;
                        default: hit = walk_longest_vcs<SHADOW, false, 2, 1, 0>(oo, ds, pc, reg, tail, hcol, hcode); break;
                    }
                }
            }
        }
        if (aborted) return false;
        // the original-DDA tail; a shadow walk of an equal-component light takes the
        // one-division loop (grid_original's EQ)
        if (tail)
            return grid_original_rt(oo, od, reg, cr, h, SHADOW, SHADOW && VR_LONG_TAIL_EQ && v.L_eq, nullptr, nullptr,
                                    VR_LONG_TAIL_GENERIC);
        if (!SHADOW && hit) {
            const float one = (hcode & 4u) ? 1.0f : -1.0f;
            const uint32_t a = hcode & 3u;
            h.col = hcol;
            h.nc = this->ncode(a, one);
            h.so = oo;
            h.region = cr;
            h.longest = true;
        }
        return hit;
    }

    // rayMarchVoxelScene (Renderer.cuh:338-434) / rayMarchVoxelSceneLongestAxis (:917-1010).
    template <int ALGO>
    __device__ __forceinline__ bool primary(f3 wo, f3 wd, Hit& h) {
        f3 tr = ld3(v.translation);
        f3 so = scl(v.scale_f, sub(wo, tr));      // Ray::convertRayToLocalSpace (Ray.cuh:14-17)
        f3 d = wd;
        // the ray's reciprocals, made once for every division by d in the entry clip
        // (div_fast) and, cuckoo store only (see kFastSetup), in the region walks
        const Rcp rc[3] = {rcp_setup(d.x), rcp_setup(d.y), rcp_setup(d.z)};
        i3 cr{f2i(floorf(so.x / 64.0f)), f2i(floorf(so.y / 64.0f)), f2i(floorf(so.z / 64.0f))};
        VR_DIAG_COUNT(14);                            // primary() calls
        auto cyc = this->cycle_start(cr, so);     // (kExact only: dead code in the tile pass)
        while (!in_scene(cr)) {                   // entry clip (:349-373)
            if (!tick()) return false;
            VR_DIAG_COUNT(15);
            int32_t hi = (int32_t)(s.D + (uint32_t)s.min_coord), lo = s.min_coord;
            int32_t nx = d.x < 0.0f ? hi : lo, ny = d.y < 0.0f ? hi : lo, nz = d.z < 0.0f ? hi : lo;
            const float ax = (float)(nx * kBlock) - so.x, ay = (float)(ny * kBlock) - so.y,
                        az = (float)(nz * kBlock) - so.z;
            float tX = div_fast(ax, rc[0]), tY = div_fast(ay, rc[1]), tZ = div_fast(az, rc[2]);
            // (a numerator is never -0 here; +0 divides exactly)
            const bool fast = (__float_as_uint(ax) == 0u || div_fast_ok(ax, rc[0])) &&
                              (__float_as_uint(ay) == 0u || div_fast_ok(ay, rc[1])) &&
                              (__float_as_uint(az) == 0u || div_fast_ok(az, rc[2]));
            if (__builtin_expect(__builtin_amdgcn_ballot_w64(!fast) != 0, 0)) {
                VR_DIAG_COUNT(39);                     // entry clip: a lane outside div_fast's domain
                tX = fast ? tX : ax / d.x;
                tY = fast ? tY : ay / d.y;
                tZ = fast ? tZ : az / d.z;
            }
            if (tX <= 0.0f) tX = kInf;
            if (tY <= 0.0f) tY = kInf;
            if (tZ <= 0.0f) tZ = kInf;
            float tMin = fminf(tX, fminf(tY, tZ));
            if (tMin == kInf) return false;
            so = add(so, scl(tMin + kEps, d));
            cr = i3{f2i(floorf(so.x / 64.0f)), f2i(floorf(so.y / 64.0f)), f2i(floorf(so.z / 64.0f))};
            if (kExact && this->cycle_step(cyc, cr, so)) { aborted = true; return false; }   // never ends
        }
        f3 o = sub(so, mk((float)(cr.x * kBlock), (float)(cr.y * kBlock), (float)(cr.z * kBlock)));
        return primary_regions<ALGO>(o, d, cr, h, nullptr, rc);
    }
    // The tile pass's original shadow walk dispatches on the light's sign pattern once per ray.
    static constexpr bool kShadowArms = VR_SHADOW_ARMS && !CRAWL;
    // Run f in the arm of the uniform sign pattern sg (bit 0: d.x > 0, bit 1: y, bit 2: z):
    // f(Sgn<+-1>..., ArmRay) -- for pattern 7, Sgn<2> three times when walk_ok holds.  sg and
    // walk_ok are the light's, the same in every lane: the branches are scalar (s_cmp,
    // s_cbranch_scc), no lane mask is made.  EQ (equal components): only patterns 0 and 7 exist.
    template <bool EQ, class F>
    __device__ __forceinline__ bool arms(uint32_t sg, bool walk_ok, F&& f) {
        const uint32_t p = __builtin_amdgcn_readfirstlane(sg);
        ArmRay aw;
        aw.nlim = walk_ok ? 0x1p-90f : kInf;
        aw.okw = walk_ok;
        using N = Sgn<-1>;
        using P = Sgn<1>;
        using Q = Sgn<2>;
        if (p == 7u) {
            if (aw.okw) return f(Q{}, Q{}, Q{}, aw);
            VR_DIAG_COUNT(42);         // a lane's walk_ok failed: P,P,P with checks
            return f(P{}, P{}, P{}, aw);
        }
        if (p == 0u) return f(N{}, N{}, N{}, aw);
        if constexpr (!EQ) {
            switch (p) {
            case 1: return f(P{}, N{}, N{}, aw);
            case 2: return f(N{}, P{}, N{}, aw);
            case 3: return f(P{}, P{}, N{}, aw);
            case 4: return f(N{}, N{}, P{}, aw);
            case 5: return f(P{}, N{}, P{}, aw);
            default: return f(N{}, P{}, P{}, aw);
            }
        }
        return false;
    }
    // The region walk of rayMarchVoxelScene(LongestAxis) (:376-433); rs (crawl
    // pass): first finish the region walk a deferral record left at its crawl.
    template <int ALGO>
    __device__ __forceinline__ bool primary_regions(f3 o, f3 d, i3 cr, Hit& h, const uint32_t* rs,
                                                    const Rcp* rc = nullptr) {
        if (CRAWL && rs != nullptr) {
            const bool hit = grid_original_rt(o, d, this->region_at_nocount(cr), cr, h, false, false, rs);
            if (aborted) return false;
            if (hit) return true;
            advance_region(cr, o);
        }
        auto cyc = this->cycle_start(cr, o);
        while (in_scene(cr)) {
            // (VCS longest axis: the direction is made opaque per region round, so the walk's
            // per-direction values -- longest-axis frame, sign classes, the tail's plane signs --
            // are made inside the round instead of hoisted out of it and kept live through every
            // walk, which spilled them: VR_LONG_REMAT)
            if (kRematDir && ALGO == ALGO_LONGEST) asm volatile("" : "+v"(d.x), "+v"(d.y), "+v"(d.z));
            if (!tick()) return false;
            VR_DIAG_COUNT(10);                         // primary region rounds
            uint32_t reg = region_at(cr);
            auto cyc1 = this->cycle_start(cr, o);
            while (reg == kNone) {
                if (!tick()) return false;
                VR_DIAG_COUNT(11);                     // null-region skips
                if (!this->template skip_null<false>(cr, o, d, reg)) return false;
                // kExact: a loop whose state repeats never ends (the reference never
                // returns); the VCS tile pass hands such pixels over through its budget
                if (kExact && this->cycle_step(cyc1, cr, o)) { aborted = true; return false; }
            }
            bool hit = ALGO == ALGO_ORIGINAL ? grid_original<false>(o, d, reg, cr, h, nullptr, rc)
                                             : (STORE == STORE_VCS ? grid_longest_vcs<false>(o, d, reg, cr, h)
                                                                   : grid_longest<false>(o, d, reg, cr, h));
            if (aborted) return false;
            if (hit) return true;
            advance_region(cr, o);
            if (kExact && this->cycle_step(cyc, cr, o)) { aborted = true; return false; }
        }
        return false;
    }

    // isInShadowOriginalRayMarch (Renderer.cuh:174-235) /
    // isInShadowRayMarchVoxelSceneLongestAxis (:633-694).
    // ARMS: dispatch on the light's sign pattern here, once per ray (see arms).  The original
    // algorithm's tile pass asks for it; the longest-axis kernel, whose rare original-DDA hits
    // also come here, keeps the dispatch per round (less code in a kernel that spills: with the
    // arms C3 ran 0.1791 -> 0.1840 ms per frame in flight, profiles/setup/).
    template <bool LONGEST, bool EQ = false, bool ARMS = false>
    __device__ __forceinline__ bool shadow(f3 o, i3 cr, const uint32_t* rs = nullptr) {
        f3 d = ld3(v.L);
        // the light's reciprocals, made on the host (uniform: SGPRs, no VGPRs)
        const bool lf = v.L_fast != 0u;
        const Rcp rc[3] = {Rcp{d.x, v.Lr[0], lf}, Rcp{d.y, v.Lr[1], lf}, Rcp{d.z, v.Lr[2], lf}};
        if constexpr (kShadowArms && ARMS && !LONGEST) {
            // the light's sign pattern and walk_ok are uniform: scalar branches to its arm
            const uint32_t sg = (d.x > 0.0f ? 1u : 0u) | (d.y > 0.0f ? 2u : 0u) | (d.z > 0.0f ? 4u : 0u);
            const bool walk_ok = lf && d.x != 0.0f && d.y != 0.0f && d.z != 0.0f;
            return arms<EQ>(sg, walk_ok, [&](auto ax, auto ay, auto az, const ArmRay& aw) __attribute__((always_inline)) {
                return shadow_regions<LONGEST, EQ, decltype(ax)::value, decltype(ay)::value, decltype(az)::value>(
                    o, d, cr, nullptr, rc, &aw);
            });
        } else {
            return shadow_regions<LONGEST, EQ>(o, d, cr, rs, rc);
        }
    }
    template <bool LONGEST, bool EQ, int AX = 0, int AY = 0, int AZ = 0>
    __device__ __forceinline__ bool shadow_regions(f3 o, f3 d, i3 cr, const uint32_t* rs, const Rcp* rc,
                                                   const ArmRay* aw = nullptr) {
        Hit dummy;
        if (CRAWL && rs != nullptr) {            // resume a deferred crawl (as primary_regions)
            const bool hit = grid_original_rt(o, d, this->region_at_nocount(cr), cr, dummy, true, EQ, rs);
            if (aborted) return false;
            if (hit) return true;
            advance_region(cr, o);
        }
        auto cyc = this->cycle_start(cr, o);
        while (in_scene(cr)) {
            if (kRematDir && LONGEST) asm volatile("" : "+s"(d.x), "+s"(d.y), "+s"(d.z));   // (see primary_regions; uniform)
            if (!tick()) return false;
            VR_DIAG_COUNT(12);                         // shadow region rounds
            uint32_t reg = region_at(cr);
            auto cyc1 = this->cycle_start(cr, o);
            while (reg == kNone) {
                if (!tick()) return false;
                VR_DIAG_COUNT(13);
                if (!this->template skip_null<!LONGEST>(cr, o, d, reg)) return false;
                if (kExact && this->cycle_step(cyc1, cr, o)) { aborted = true; return false; }   // (as above)
            }
            bool hit;
            if constexpr (AX != 0)
                hit = this->template grid_original_rt<AX, AY, AZ>(o, d, reg, cr, dummy, true, EQ, nullptr, rc, false, aw);
            else
                hit = LONGEST ? (STORE == STORE_VCS ? grid_longest_vcs<true>(o, d, reg, cr, dummy)
                                                    : grid_longest<true>(o, d, reg, cr, dummy))
                              : grid_original<true, EQ>(o, d, reg, cr, dummy, nullptr, rc);
            if (aborted) return false;
            if (hit) return true;
            advance_region(cr, o);
            if (kExact && this->cycle_step(cyc, cr, o)) { aborted = true; return false; }
        }
        return false;
    }
};

// applyLighting at the primary hit (Renderer.cuh:249-258; regionWorldPosition :413)
// times !shadow (:315,737,821): the pixel's colour.
// (ALGO: the original algorithm's kernels take the shadow walk's sign arms, Walker::shadow)
// W: any Walker -- the render's (vr_march.hip) or, with PICK, the shade kernel's (vr_shade.hip).
template <int ALGO, class W>
__device__ __forceinline__ uint32_t light_and_shadow(W& w, const KView& v, const Hit& h) {
    constexpr bool kArms = ALGO == ALGO_ORIGINAL;
    bool sh = false;
    const f3 rwp = add(ld3(v.translation), mk((float)(h.region.x * kBlock), (float)(h.region.y * kBlock),
                                              (float)(h.region.z * kBlock)));
    const uint32_t lit = w.lighting(h.col, h.nc, rwp, h.so);
    if (v.use_shadows) {
        VR_DIAG_COUNT(16);                             // shadow walks started
        w.lit_saved = lit;
        const bool eq = v.L[0] == v.L[1] && v.L[1] == v.L[2];
        if (h.longest) {
            w.ctx = 2u;
            sh = w.template shadow<true>(h.so, h.region);
        } else {
            sh = eq ? w.template shadow<false, true, kArms>(h.so, h.region)
                    : w.template shadow<false, false, kArms>(h.so, h.region);
        }
    }
    return lit * (uint32_t)!sh;
}

// calculateWorldRay (Renderer.cuh:1013-1022) + Camera::generateRay (Camera.cuh:25-29)
// for pixel (x, local row l); false when the row is outside the frame.
// FAST (cuckoo store, see Walker::kFastSetup): divisions with hoisted reciprocals.
template <bool FAST>
__device__ __forceinline__ bool pixel_ray(const KView& v, uint32_t x, uint32_t l, f3& ro, f3& rd) {
    // band = l / band_rows: q0 = mulhi(l, floor(2^32 / band_rows)) is q or q - 1 (see FastMod)
    const uint32_t q0 = __umulhi(l, v.band_minv), r0 = l - q0 * v.band_rows;
    const bool up = r0 >= v.band_rows;
    const uint32_t band = q0 + (up ? 1u : 0u), in_band = up ? r0 - v.band_rows : r0;
    const uint32_t y = v.row0 + (band * v.nranks + v.rank) * v.band_rows + in_band;
    if (y >= v.row_limit) return false;
    if (v.tile_cols) {
        // 2-D tile deal (uniform branch): local column -> frame column (vr_internal.h KView)
        const uint32_t j0 = __umulhi(x, v.tile_minv), r1 = x - j0 * v.tile_cols;
        const bool up1 = r1 >= v.tile_cols;
        const uint32_t j = j0 + (up1 ? 1u : 0u), in_blk = up1 ? r1 - v.tile_cols : r1;
        const uint32_t off = (v.col_rank + v.col_R - (v.col_stride * (band % v.col_R)) % v.col_R) % v.col_R;
        x = (j * v.col_R + off) * v.tile_cols + in_blk;
        if (x >= v.W) return false;
    }
    if (!FAST) {
        float u = ((float)x + 0.5f) / (float)v.W;
        float vv = ((float)(v.H - y) + 0.5f) / (float)v.H;
        ro = add(add(ld3(v.llc), scl(u, ld3(v.hor))), scl(vv, ld3(v.ver)));
        rd = unit(sub(ro, ld3(v.org)));
        return true;
    }
    // correctly rounded divisions by W, H (in [1, 65536]) and |ro - eye| with
    // hoisted reciprocals (div_fast; its domain holds for u and v: numerators
    // in [0.5, 65536])
    const Rcp rW = rcp_setup((float)v.W), rH = rcp_setup((float)v.H);
    float u = div_fast((float)x + 0.5f, rW);
    float vv = div_fast((float)(v.H - y) + 0.5f, rH);
    ro = add(add(ld3(v.llc), scl(u, ld3(v.hor))), scl(vv, ld3(v.ver)));
    const f3 c = sub(ro, ld3(v.org));                  // Vector3::normalize (Vector3.cuh:162, :79)
    const float len = sqrtf(c.x * c.x + c.y * c.y + c.z * c.z);
    const Rcp rl = rcp_setup(len);
    auto okn = [&](float n) { return __float_as_uint(n) == 0u || div_fast_ok(n, rl); };
    rd = f3{div_fast(c.x, rl), div_fast(c.y, rl), div_fast(c.z, rl)};
    VR_DIAG_COUNT_IF(!(okn(c.x) && okn(c.y) && okn(c.z)), 40);   // ray direction: IEEE fallback
    if (!(okn(c.x) && okn(c.y) && okn(c.z))) rd = f3{c.x / len, c.y / len, c.z / len};
    return true;
}

// Host side: a launcher's run-time {store, algo} as compile-time tags.  f is a generic lambda,
// called once as f(std::integral_constant<int, STORE_*>{}, std::integral_constant<int, ALGO_*>{}),
// so its body names kernel<decltype(st)::value, decltype(al)::value> and all four pairs exist.
template <class F>
inline void for_store_algo(int store, int algo, F&& f) {
    using Vcs = std::integral_constant<int, STORE_VCS>;
    using Hash = std::integral_constant<int, STORE_HASH>;
    using Orig = std::integral_constant<int, ALGO_ORIGINAL>;
    using Long = std::integral_constant<int, ALGO_LONGEST>;
    if (store == STORE_VCS) {
        if (algo == ALGO_ORIGINAL) f(Vcs{}, Orig{}); else f(Vcs{}, Long{});
    } else {
        if (algo == ALGO_ORIGINAL) f(Hash{}, Orig{}); else f(Hash{}, Long{});
    }
}

}  // namespace
}  // namespace vr
