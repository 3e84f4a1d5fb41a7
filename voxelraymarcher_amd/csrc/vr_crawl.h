// vr_crawl.h -- the closed-form fast-forward of cluster-skip crawls (crawl_steps,
// crawl_run) and the voxel recovery behind the crawl pass's resume (crawl_voxel).
// Pure float arithmetic, no memory but the region's cluster bits: compiled for the
// device with vr_walk.h, which uses it, and for both sides by tools/crawl_check.hip,
// which holds it against a plain single-step loop (tests/test_crawl_check.py).
// Two things differ between the sides: the reciprocal of crawl_floor (crawl_rcp) and
// the bit casts (crawl_bits / crawl_float: the device's __float_as_uint /
// __uint_as_float, which the host has not).
#pragma once
#include "vr_device.h"

#include <math.h>
#include <string.h>

namespace vr {
namespace {

__host__ __device__ __forceinline__ float crawl_rcp(float den) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rcpf(den);
#else
    return 1.0f / den;
#endif
}
__host__ __device__ __forceinline__ uint32_t crawl_bits(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(f);
#else
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
#endif
}
__host__ __device__ __forceinline__ float crawl_float(uint32_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float f;
    memcpy(&f, &u, 4);
    return f;
#endif
}

// Exact fast-forward of a cluster-skip crawl (rayMarchVoxelGrid's skip branch,
// Renderer.cuh:290-306, with tMin = +-0).  An iteration started in an absent
// cluster, found t = 0 on an axis whose skip plane is the position itself and
// moved to `on` = o + RN(EPSILON * d) componentwise.  While the positions stay
// in that cluster and, per axis, in one binade, every further iteration is the
// same skip: t = 0 on the same (unmoved) axis -- every other t is >= 0 -- and
// o_i <- RN(o_i + c_i), c_i = RN(EPSILON * d_i), i.e. o_i += delta_i, a fixed
// multiple of the binade's ulp (for a tie c_i / ulp = k + 1/2 only from an even
// mantissa, where every step lands on an even mantissa again).  Returns the number
// m of such iterations (0 = none, at most `room`) and the per-axis deltas; the
// caller credits m loop iterations and m existence reads.
struct Crawl { uint32_t m; float dx, dy, dz; };
// One axis: returns false to decline; else sets its delta, ORs in whether it is
// pinned on its skip plane, and lowers m to a number of iterations its binade and
// the cluster certainly allow (the float quotients are shrunk by 2^-20, so m may
// come out a little low -- the walk then simply runs those iterations -- never high).
__host__ __device__ __forceinline__ float crawl_floor(float num, float den) {
    return floorf(num * crawl_rcp(den) * (1.0f - 0x1p-20f));
}
__host__ __device__ __forceinline__ bool crawl_axis(float x, float dir, int32_t v, bool pos, float& delta, bool& pinned,
                                                    float& m) {
    const float c = kEps * dir, nx = x + c;
    const float cl = (float)(v & ~7);                                           // cluster [cl, cl + 8)
    if (nx == x) {
        delta = 0.0f;
        pinned |= !pos && cl == x;
        return true;
    }
    if (!(x >= 0x1p-100f)) return false;     // zero / tiny coordinate: no binade arithmetic
    const uint32_t bits = crawl_bits(x), be = bits >> 23;                       // x > 0: biased exponent
    const float lo = crawl_float(be << 23), hi = crawl_float((be + 1u) << 23);
    if (!(nx >= lo && nx < hi)) return false;
    const float x1 = crawl_float(bits + 1u), x2 = crawl_float(bits + 2u);
    delta = nx - x;                           // exact (same binade)
    if (!(x2 < hi)) return false;
    if ((x1 + c) - x1 != delta) {
        // c / ulp = k + 1/2: ties-to-even makes every result's mantissa even, so
        // from an even mantissa the step is constant (checked on the next even one).
        if ((bits & 1u) || (x2 + c) - x2 != delta) return false;
    }
    // positions x + t*delta: t = 0..m inside [lo, hi), t = 0..m-1 inside [cl, cl + 8)
    m = delta > 0.0f ? fminf(m, fminf(crawl_floor(hi - x, delta), crawl_floor(cl + 8.0f - x, delta)))
                     : fminf(m, fminf(crawl_floor(x - lo, -delta), crawl_floor(x - cl, -delta)));
    return true;
}
__host__ __device__ __forceinline__ Crawl crawl_steps(f3 on, f3 d, int32_t vx, int32_t vy, int32_t vz,
                                                      bool px, bool py, bool pz, uint32_t room) {
    Crawl r{0u, 0.0f, 0.0f, 0.0f};
    if (((f2i(on.x) ^ vx) | (f2i(on.y) ^ vy) | (f2i(on.z) ^ vz)) & ~7) return r;   // left the cluster
    if (!(on.x >= 0.0f && on.y >= 0.0f && on.z >= 0.0f)) return r;
    bool pinned = false;
    float m = (float)room;
    f3 dl{0.0f, 0.0f, 0.0f};
    // (crawl kernel only: its register budget is not the tile pass's, so the axes are
    // unrolled -- VR_CRAWL_ROLLED keeps the rolled loop for A/B)
#ifdef VR_CRAWL_ROLLED
#pragma unroll 1
#else
#pragma unroll
#endif
    for (uint32_t a = 0; a < 3u; ++a) {
        float delta;
        if (!crawl_axis(comp(on, a), comp(d, a), a == 0 ? vx : (a == 1 ? vy : vz), a == 0 ? px : (a == 1 ? py : pz),
                        delta, pinned, m))
            return r;
        setf(dl, a, delta);
    }
    r.m = (pinned && m > 0.0f) ? (uint32_t)m : 0u;
    r.dx = dl.x; r.dy = dl.y; r.dz = dl.z;
    return r;
}

// A whole crawl (crawl pass): from `o` -- the position a crawl iteration stepped to from
// voxel q -- apply every further crawl iteration: runs of identical steps in one binade
// at once (crawl_steps), and the steps between runs (across a binade edge, a tie from an
// odd mantissa) one by one, exactly as the walk computes them, o_i + RN(EPSILON * d_i).
// Returns their number (0: not a crawl); at most `room`.  Pure arithmetic: a crawl of
// 10^5..10^6 iterations costs a few dozen loop trips instead of as many dependent mask
// loads.
//   lbm == null (performVoxelSpaceJump's crawls): only the iterations whose results stay
// in q's cluster; the step that leaves it is left to the walk (the jump's hit normal
// reads its t values).
//   lbm (the original DDA's crawls, whose skip steps feed no normal: Renderer.cuh:297-301,
// SURVEY Q8): the region's cluster-existence bits.  A crawl does not end at its cluster's
// face: an iteration that starts in an ABSENT cluster with the pinned axis still on its
// plane (it never moves; the next cluster on the other axes shares that plane) is again a
// skip with t = +-0 -- the same step.  So the crossing step is taken here as well, and
// the crawl goes on through every absent cluster the ray meets in the region; it stops
// after the step into a present cluster or out of the region (the walk resumes there).
// Without this, each face crossing returned to the walk loop, which re-armed crawl
// detection only after 8 single-step iterations: ~10-35 crossings per C5 record.
__host__ __device__ __forceinline__ uint32_t crawl_run(f3& o, f3 d, int32_t qx, int32_t qy, int32_t qz, bool px,
                                                       bool py, bool pz, uint32_t room, const uint32_t* lbm = nullptr,
                                                       uint32_t* trips = nullptr) {
    const f3 c{kEps * d.x, kEps * d.y, kEps * d.z};
    int32_t lx = qx & ~7, ly = qy & ~7, lz = qz & ~7;
    // an axis pinned on its cluster plane: direction negative, on the plane, unmoved by its step
    const bool pinned = (!px && (float)lx == o.x && o.x + c.x == o.x) ||
                        (!py && (float)ly == o.y && o.y + c.y == o.y) ||
                        (!pz && (float)lz == o.z && o.z + c.z == o.z);
    if (!pinned) return 0u;
    auto inside = [&](f3 p) {   // in the cluster [l, l + 8) on every axis (p >= 0: trunc = floor)
        return p.x >= (float)lx && p.x < (float)(lx + 8) && p.y >= (float)ly && p.y < (float)(ly + 8) &&
               p.z >= (float)lz && p.z < (float)(lz + 8);
    };
    // p left the current cluster: go on crawling in p's cluster when it is in the region and absent
    auto absent_next = [&](f3 p) -> bool {
        if (!lbm || !(p.x >= 0.0f && p.x < 64.0f && p.y >= 0.0f && p.y < 64.0f && p.z >= 0.0f && p.z < 64.0f))
            return false;
        const int32_t ax = f2i(p.x), ay = f2i(p.y), az = f2i(p.z);
        const uint32_t slot = (uint32_t)(((az >> 3) << 6) | ((ay >> 3) << 3) | (ax >> 3));
        if ((lbm[slot >> 5] >> (slot & 31u)) & 1u) return false;
        qx = ax; qy = ay; qz = az;
        lx = ax & ~7; ly = ay & ~7; lz = az & ~7;
        return true;
    };
    if (!inside(o) && !absent_next(o)) return 0u;   // the crawl iteration itself left the cluster
    uint32_t n = 0;
#pragma unroll 1
    for (uint32_t trip = 0; trip < 65536u && n < room; ++trip) {
        if (trips) ++*trips;
        const Crawl cw = crawl_steps(o, d, qx, qy, qz, px, py, pz, room - n);
        if (cw.m != 0u) {
            const float fm = (float)cw.m;       // exact: m * delta_i stays inside the binade
            o = f3{o.x + fm * cw.dx, o.y + fm * cw.dy, o.z + fm * cw.dz};
            n += cw.m;
            if (n >= room) break;
        }
        const f3 o1{o.x + c.x, o.y + c.y, o.z + c.z};
        if (!inside(o1)) {
            if (!lbm) break;
            o = o1;                             // the crossing step (a skip in an absent cluster)
            ++n;
            if (!absent_next(o1)) break;
            continue;
        }
        o = o1;
        ++n;
    }
    return n;
}

// A crawl iteration has t = 0, so it stepped o_i <- RN(o_i + c_i), c_i =
// RN(EPSILON d_i); its voxel is q_i = trunc(old o_i), old o_i >= 0 (it was in
// the region).  The old coordinate lies within ulp(on)/2 + ulp(e)/2 of
// e = RN(on - c) (< 1.5 ulp(e) for e >= 1), so it is one of the floats at most 4
// steps from e that step to `on`: q is found when all of those truncate alike.
__host__ __device__ __forceinline__ bool crawl_voxel(float on, float c, int32_t& q) {
    const float e = on - c;
    if (e + 0x1p-20f < 1.0f) { q = 0; return true; }          // every candidate in [0, 1)
    int32_t found = -1;
    bool ok = true;
#pragma unroll 1
    for (int32_t k = -4; k <= 4; ++k) {
        const float x = crawl_float(crawl_bits(e) + (uint32_t)k);
        if (!(x >= 0.0f) || x + c != on) continue;
        const int32_t t = f2i(x);
        ok &= found < 0 || t == found;
        found = t;
    }
    q = found;
    return ok && found >= 0;
}

}  // namespace
}  // namespace vr
