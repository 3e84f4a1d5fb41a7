// crawl_check -- the closed-form crawl fast-forward (vr_crawl.h: crawl_steps, crawl_run,
// crawl_voxel) against a plain single-step loop, o <- o + RN(EPSILON d) per component in
// float32, written here without a trip cap and without a call into the header.  Built with
// the library's flags (no contraction, no fast-math).  Prints one JSON line; exit 0 iff
// every check holds, 1 otherwise (2: a HIP call failed).
//   crawl_check [--cpu] [cases] [seed]
// Default: the header's device compile -- one lane per case, results copied back and
// compared on the host.  --cpu: the header's host compile; no HIP runtime call is made.
//
// Per case and mode (without / with the region's cluster bits), n_fast = crawl_run's count:
//   1. exact prefix: n_fast <= room, and the loop run with room = n_fast returns n_fast
//      and a bit-identical position;
//   2. complete: n_fast = the loop's count for the case's room, or the trip cap ended the
//      run early (n_fast >= 65536 -- every trip yields an iteration -- and n_fast < n_ref):
//      at most 1 % of the cases;
//   3. it fast-forwards: of the runs with n_ref >= 1000, 95 % take <= n_ref / 100 trips;
//   4. crawl_steps alone from the same start: m > 0 means that m single steps from `on`
//      land exactly on on + m * delta per axis, leave a pinned axis where it was and keep
//      positions 0..m-1 in q's cluster.
// The generator is part of the test: n_ref = 0 in at most 30 % of the runs, and at least
// 20 % end by themselves (0 < n_ref < room: they left the cluster, met a present one or
// left the region).  crawl_voxel: for on = RN(o_prev + c) it reports ambiguity or returns
// trunc(o_prev) (the three input families of tests/test_crawl_voxel.py).
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../vr_crawl.h"

namespace {

struct Case {
    float o[3], d[3];
    int32_t q[3];
    uint32_t room;
    uint32_t bm[16];     // the region's 512 cluster bits: slot = z >> 3 << 6 | y >> 3 << 3 | x >> 3
};
struct Run { uint32_t n, trips; float o[3]; };
struct Out {
    Run run[2];          // crawl_run without / with the cluster bits
    uint32_t m;          // crawl_steps
    float dl[3];
};

// ---------------------------------------------------------------- code under test
__host__ __device__ inline void fast_case(const Case& k, Out& r) {
    const vr::f3 d{k.d[0], k.d[1], k.d[2]};
    const bool px = d.x > 0.0f, py = d.y > 0.0f, pz = d.z > 0.0f;
    for (int mode = 0; mode < 2; ++mode) {
        vr::f3 o{k.o[0], k.o[1], k.o[2]};
        uint32_t trips = 0;
        const uint32_t n = vr::crawl_run(o, d, k.q[0], k.q[1], k.q[2], px, py, pz, k.room,
                                         mode ? k.bm : nullptr, &trips);
        r.run[mode] = Run{n, trips, {o.x, o.y, o.z}};
    }
    const vr::Crawl cw = vr::crawl_steps(vr::f3{k.o[0], k.o[1], k.o[2]}, d, k.q[0], k.q[1], k.q[2], px, py, pz, k.room);
    r.m = cw.m;
    r.dl[0] = cw.dx; r.dl[1] = cw.dy; r.dl[2] = cw.dz;
}
constexpr int32_t kAmbiguous = INT32_MIN;
__host__ __device__ inline int32_t fast_voxel(float on, float c) {
    int32_t q;
    return vr::crawl_voxel(on, c, q) ? q : kAmbiguous;
}

__global__ void run_cases(const Case* cs, Out* out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) fast_case(cs[i], out[i]);
}
__global__ void run_voxels(const float* on, const float* c, int32_t* q, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) q[i] = fast_voxel(on[i], c[i]);
}

// ---------------------------------------------------------------- the reference
constexpr float kStep = 0.0001f;     // EPSILON

uint32_t fbits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
float bitsf(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

bool in_cluster(const float* p, const int32_t* K) {
    for (int a = 0; a < 3; ++a)
        if (!(p[a] >= (float)K[a] && p[a] < (float)(K[a] + 8))) return false;
    return true;
}
bool in_region(const float* p) {
    for (int a = 0; a < 3; ++a)
        if (!(p[a] >= 0.0f && p[a] < 64.0f)) return false;
    return true;
}
void cluster_of(const float* p, int32_t* K) {        // p in the region
    for (int a = 0; a < 3; ++a) K[a] = (int32_t)floorf(p[a]) & ~7;
}
bool present(const uint32_t* bm, const int32_t* K) {
    const uint32_t slot = (uint32_t)(((K[2] >> 3) << 6) | ((K[1] >> 3) << 3) | (K[0] >> 3));
    return (bm[slot >> 5] >> (slot & 31u)) & 1u;
}

struct Ref { uint32_t n; float o[3]; };
Ref ref_crawl(const Case& k, uint32_t room, bool bits) {
    Ref r{0u, {k.o[0], k.o[1], k.o[2]}};
    float c[3];
    int32_t K[3];
    bool pinned = false;
    for (int a = 0; a < 3; ++a) {
        c[a] = kStep * k.d[a];
        K[a] = k.q[a] & ~7;
        pinned |= !(k.d[a] > 0.0f) && r.o[a] == (float)K[a] && r.o[a] + c[a] == r.o[a];
    }
    if (!pinned) return r;
    if (!in_cluster(r.o, K)) {
        if (!bits || !in_region(r.o)) return r;
        cluster_of(r.o, K);
        if (present(k.bm, K)) return r;
    }
    while (r.n < room) {
        const float o1[3] = {r.o[0] + c[0], r.o[1] + c[1], r.o[2] + c[2]};
        if (!in_cluster(o1, K)) {
            if (!bits) break;
            memcpy(r.o, o1, sizeof o1);
            ++r.n;
            if (!in_region(o1)) break;
            cluster_of(o1, K);
            if (present(k.bm, K)) break;
            continue;
        }
        memcpy(r.o, o1, sizeof o1);
        ++r.n;
    }
    return r;
}

// ---------------------------------------------------------------- the generator
struct Rng {
    uint64_t s;
    uint64_t next() {      // splitmix64
        s += 0x9E3779B97F4A7C15ull;
        uint64_t z = s;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    double uni() { return (double)(next() >> 11) * 0x1p-53; }           // [0, 1)
    uint32_t below(uint32_t n) { return (uint32_t)(next() % n); }
    int range(int lo, int hi) { return lo + (int)below((uint32_t)(hi - lo + 1)); }
};

// x moved by k floats (x >= 0; below +0 the negative floats follow)
float nudge(float x, int k) {
    const int64_t b = (int64_t)fbits(x) + k;
    return b >= 0 ? bitsf((uint32_t)b) : -bitsf((uint32_t)(-b));
}
float ulp_of(float x) { return nudge(x, 1) - x; }                       // x > 0

float coordinate(Rng& g) {
    switch (g.below(5)) {
    case 0: return (float)(g.uni() * 64.0);
    case 1: return nudge(ldexpf(1.0f, g.range(-3, 6)), g.range(-40, 40));      // next to a power of two
    case 2: return nudge((float)(8 * g.range(0, 8)), g.range(-30, 30));        // next to a cluster face
    case 3:
        switch (g.below(4)) {
        case 0: return 0.0f;
        case 1: return ldexpf((float)(1.0 + g.uni()), -g.range(101, 149));     // below 2^-100, subnormals too
        case 2: return (float)g.uni();
        default: return ldexpf((float)(1.0 + g.uni()), -g.range(1, 30));
        }
    default: return (float)g.range(0, 63);
    }
}
float direction(Rng& g) {   // 1e-6 .. 1, either sign
    const float m = (float)pow(10.0, -6.0 * g.uni());
    return g.below(2) ? m : -m;
}
// d with RN(EPSILON d) = +-(k + 1/2) ulp(x), 1e-6 <= |d| <= 1: the ties-to-even branch
bool tie_direction(Rng& g, float x, float& d) {
    if (!(x >= 0x1p-20f)) return false;
    const float u = ulp_of(x), sgn = g.below(2) ? 1.0f : -1.0f;
    for (int t = 0; t < 16; ++t) {
        const float c = ((float)g.range(0, 50) + 0.5f) * u;                     // exact
        const float d0 = c / kStep;
        if (!(d0 >= 1e-6f && d0 <= 1.0f)) continue;
        for (int j = -3; j <= 3; ++j) {
            const float dj = nudge(d0, j);
            if (kStep * dj == c) { d = sgn * dj; return true; }
        }
    }
    return false;
}

int32_t voxel_of(float x) { return x >= 0.0f && x < 64.0f ? (int32_t)x : (x >= 64.0f ? 63 : 0); }

Case make_case(Rng& g) {
    Case k{};
    const int a = (int)g.below(3), plane = 8 * g.range(0, 7);
    // room: a quarter in 1..300, the others log-uniform up to 2^17
    k.room = g.below(4) == 0 ? 1u + g.below(300) : (uint32_t)exp2(17.0 * g.uni());
    if (k.room < 1u) k.room = 1u;
    if (k.room > (1u << 17)) k.room = 1u << 17;
    for (int b = 0; b < 3; ++b) {
        if (b == a) continue;
        k.o[b] = coordinate(g);
        k.d[b] = direction(g);
    }
    // the pinned axis: on a cluster plane, direction -0 or negative and too small to move it
    k.o[a] = (float)plane;
    if (plane == 0 || g.below(4) == 0) {
        k.d[a] = g.below(2) ? -0.0f : -1e-42f;                                   // EPSILON d = -0
    } else {
        const float below = k.o[a] - nudge(k.o[a], -1);
        float d = -(float)((double)below * 0.5 / kStep * 0.99 * pow(10.0, -4.0 * g.uni()));
        while (k.o[a] + kStep * d != k.o[a]) d *= 0.5f;
        k.d[a] = d;
    }
    const int b0 = (a + 1 + (int)g.below(2)) % 3;        // one of the two free axes
    if (g.below(8) == 0) tie_direction(g, k.o[b0], k.d[b0]);
    // near the exit: within room * |c| of the face the ray leaves its cluster through
    int32_t exit_cluster[3] = {-1, -1, -1};
    if (g.below(100) < 45) {
        const int b = (a + 1 + (int)g.below(2)) % 3;
        const float c = kStep * k.d[b], x = k.o[b];
        if (c != 0.0f && x >= 0.0f && x < 64.0f) {
            const float lo = (float)((int32_t)x & ~7);
            const double dist = g.uni() * (double)k.room * fabs((double)c);
            if (dist < 7.9) {
                k.o[b] = c > 0.0f ? (float)(lo + 8.0 - dist) : (float)(lo + dist);
                for (int e = 0; e < 3; ++e) exit_cluster[e] = voxel_of(k.o[e]) & ~7;
                exit_cluster[b] += c > 0.0f ? 8 : -8;
            }
        }
    }
    // q: the voxel of the position, or (a quarter) of the position one step earlier
    const bool earlier = g.below(4) == 0;
    for (int b = 0; b < 3; ++b) k.q[b] = voxel_of(earlier ? k.o[b] - kStep * k.d[b] : k.o[b]);
    k.q[a] = plane;
    // the cluster bits: density 0 .. 0.5, q's own cluster absent; behind an aimed-at exit
    // face a present cluster half of the time
    const double density = 0.5 * g.uni();
    for (uint32_t s = 0; s < 512u; ++s)
        if (g.uni() < density) k.bm[s >> 5] |= 1u << (s & 31u);
    auto slot = [](const int32_t* K) { return (uint32_t)(((K[2] >> 3) << 6) | ((K[1] >> 3) << 3) | (K[0] >> 3)); };
    if (exit_cluster[0] >= 0 && exit_cluster[1] >= 0 && exit_cluster[2] >= 0 && exit_cluster[0] < 64 &&
        exit_cluster[1] < 64 && exit_cluster[2] < 64 && g.below(2)) {
        const uint32_t s = slot(exit_cluster);
        k.bm[s >> 5] |= 1u << (s & 31u);
    }
    const uint32_t s = slot(k.q);
    k.bm[s >> 5] &= ~(1u << (s & 31u));
    return k;
}

Case fixed_case(float ox, float oy, float oz, float dx, float dy, float dz, uint32_t room) {
    Case k{};
    k.o[0] = ox; k.o[1] = oy; k.o[2] = oz;
    k.d[0] = dx; k.d[1] = dy; k.d[2] = dz;
    for (int b = 0; b < 3; ++b) k.q[b] = voxel_of(k.o[b]);
    k.room = room;
    return k;      // no cluster present: the crawl ends at the region's face
}
// Cases kept by hand (a case that ever failed is added here).
void fixed_cases(std::vector<Case>& cs) {
    cs.push_back(fixed_case(8.0f, 3.5f, 3.25f, -1e-3f, 0.5f, 0.25f, 1u << 17));          // plain crawl
    cs.push_back(fixed_case(5.5f, 0.0f, 7.25f, 0.3f, -0.0f, -0.2f, 100000u));            // plane 0, d = -0
    cs.push_back(fixed_case(33.0f, 16.0f, 0x1p-120f, 1.5f * 0x1p-18f / kStep, -2e-3f, 1e-6f, 70000u));   // tie, tiny z
    cs.push_back(fixed_case(0x1.fffffep+4f, 40.0f, 63.5f, 0.9f, -1e-3f, 0.7f, 5000u));   // binade edge, region exit
    cs.push_back(fixed_case(16.0f, 0x1.000002p+3f, 1.0f, 1e-6f, -1e-6f, -3e-3f, 1u << 17));   // steps below an ulp
}

// ---------------------------------------------------------------- the checks
struct Tally {
    uint64_t runs = 0, over_room = 0, bad_prefix = 0, incomplete = 0, capped = 0, zero = 0, self_end = 0, long_runs = 0,
             long_fast = 0, ref_iters = 0;
};

void print_case(const char* what, const Case& k, int mode, const Run* f, const Ref* r) {
    fprintf(stderr, "%s: mode %d o (%a, %a, %a) d (%a, %a, %a) q (%d, %d, %d) room %u\n  bits", what, mode, k.o[0], k.o[1],
            k.o[2], k.d[0], k.d[1], k.d[2], k.q[0], k.q[1], k.q[2], k.room);
    for (int i = 0; i < 16; ++i) fprintf(stderr, " %08x", k.bm[i]);
    fprintf(stderr, "\n");
    if (f) fprintf(stderr, "  fast n %u trips %u o (%a, %a, %a)\n", f->n, f->trips, f->o[0], f->o[1], f->o[2]);
    if (r) fprintf(stderr, "  loop n %u o (%a, %a, %a)\n", r->n, r->o[0], r->o[1], r->o[2]);
}

bool same_pos(const float* a, const float* b) {
    return fbits(a[0]) == fbits(b[0]) && fbits(a[1]) == fbits(b[1]) && fbits(a[2]) == fbits(b[2]);
}

void check_run(const Case& k, int mode, const Run& f, Tally& t, int& shown) {
    const Ref full = ref_crawl(k, k.room, mode != 0);
    ++t.runs;
    t.ref_iters += full.n;
    t.zero += full.n == 0u;
    t.self_end += full.n > 0u && full.n < k.room;
    if (full.n >= 1000u) {
        ++t.long_runs;
        t.long_fast += (uint64_t)f.trips * 100u <= full.n;
    }
    bool bad = false;
    if (f.n > k.room) { ++t.over_room; bad = true; }
    // 1. the loop with room = n_fast (the same loop, cut short, when the counts differ)
    const Ref pre = f.n == full.n ? full : ref_crawl(k, f.n <= k.room ? f.n : k.room, mode != 0);
    if (pre.n != f.n || !same_pos(pre.o, f.o)) { ++t.bad_prefix; bad = true; }
    // 2.
    if (f.n != full.n) {
        if (f.n >= 65536u && f.n < full.n) ++t.capped;
        else { ++t.incomplete; bad = true; }
    }
    if (bad && shown < 5) { ++shown; print_case("crawl_run", k, mode, &f, &full); }
}

// 4. crawl_steps alone
bool check_steps(const Case& k, const Out& r) {
    if (r.m == 0u) return true;
    if (r.m > k.room) return false;
    const int32_t K[3] = {k.q[0] & ~7, k.q[1] & ~7, k.q[2] & ~7};
    float o[3] = {k.o[0], k.o[1], k.o[2]}, c[3];
    for (int a = 0; a < 3; ++a) c[a] = kStep * k.d[a];
    for (uint32_t i = 0; i < r.m; ++i) {
        if (!in_cluster(o, K)) return false;
        for (int a = 0; a < 3; ++a) o[a] = o[a] + c[a];
    }
    bool pinned = false;
    for (int a = 0; a < 3; ++a) {
        const double want = (double)k.o[a] + (double)r.m * (double)r.dl[a];      // exact in double
        if ((double)(float)want != want || fbits((float)want) != fbits(o[a])) return false;
        pinned |= !(k.d[a] > 0.0f) && k.o[a] == (float)K[a] && r.dl[a] == 0.0f && fbits(o[a]) == fbits(k.o[a]);
    }
    return pinned;
}

struct Voxels {
    std::vector<float> on, c;
    std::vector<int32_t> want;
    size_t n_random = 0, n_integer = 0, n_pinned = 0;
    void add(float o_prev, float d) {
        const float cc = kStep * d;
        on.push_back(o_prev + cc);
        c.push_back(cc);
        want.push_back((int32_t)o_prev);
    }
};
Voxels make_voxels(Rng& g) {
    Voxels v;
    for (int i = 0; i < 200000; ++i) v.add((float)(g.uni() * 64.0), (float)(2.0 * g.uni() - 1.0));
    v.n_random = v.on.size();
    const float mags[7] = {1e-4f, 3e-3f, 0.01f, 0.07f, 0.3f, 0.577f, 0.99f};
    for (int i = 0; i < 20000; ++i) {       // on, just below and just above integers
        const int64_t b = (int64_t)fbits((float)g.range(0, 63)) + g.range(-3, 3);
        float o = bitsf((uint32_t)(b < 0 ? 0 : b));
        if (!(o < 64.0f)) o = 63.5f;
        v.add(o, mags[g.below(7)] * (g.below(2) ? 1.0f : -1.0f));
    }
    v.n_integer = v.on.size() - v.n_random;
    const float dd[4] = {1e-3f, -1e-3f, 2e-3f, -4e-4f};
    for (int p = 8; p <= 56; p += 8)        // an axis EPSILON d cannot move: the crawl's plane
        for (int j = 0; j < 4; ++j) v.add((float)p, dd[j]);
    v.n_pinned = v.on.size() - v.n_random - v.n_integer;
    return v;
}

double seconds_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

#define CK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "%s failed\n", #x); return 2; } } while (0)

int main(int argc, char** argv) {
    bool cpu = false;
    std::vector<const char*> pos;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--cpu")) cpu = true;
        else pos.push_back(argv[i]);
    }
    const uint32_t n_random = pos.size() > 0 ? (uint32_t)strtoul(pos[0], nullptr, 0) : 20000u;
    Rng g{pos.size() > 1 ? strtoull(pos[1], nullptr, 0) : 0x5EEDC4A71ull};

    std::vector<Case> cs;
    fixed_cases(cs);
    for (uint32_t i = 0; i < n_random; ++i) cs.push_back(make_case(g));
    Voxels vx = make_voxels(g);
    const uint32_t n = (uint32_t)cs.size(), nv = (uint32_t)vx.on.size();
    std::vector<Out> out(n);
    std::vector<int32_t> vq(nv);

    const auto t_fast = std::chrono::steady_clock::now();
    if (cpu) {
        for (uint32_t i = 0; i < n; ++i) fast_case(cs[i], out[i]);
        for (uint32_t i = 0; i < nv; ++i) vq[i] = fast_voxel(vx.on[i], vx.c[i]);
    } else {
        Case* dcs = nullptr;
        Out* dout = nullptr;
        float *don = nullptr, *dc = nullptr;
        int32_t* dq = nullptr;
        CK(hipMalloc(&dcs, n * sizeof(Case)));
        CK(hipMalloc(&dout, n * sizeof(Out)));
        CK(hipMalloc(&don, nv * 4));
        CK(hipMalloc(&dc, nv * 4));
        CK(hipMalloc(&dq, nv * 4));
        CK(hipMemcpy(dcs, cs.data(), n * sizeof(Case), hipMemcpyHostToDevice));
        CK(hipMemcpy(don, vx.on.data(), nv * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(dc, vx.c.data(), nv * 4, hipMemcpyHostToDevice));
        CK(hipMemset(dout, 0xFF, n * sizeof(Out)));
        CK(hipMemset(dq, 0xFF, nv * 4));
        hipLaunchKernelGGL(run_cases, dim3((n + 63u) / 64u), dim3(64), 0, 0, dcs, dout, n);
        CK(hipGetLastError());
        hipLaunchKernelGGL(run_voxels, dim3((nv + 255u) / 256u), dim3(256), 0, 0, don, dc, dq, nv);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(out.data(), dout, n * sizeof(Out), hipMemcpyDeviceToHost));
        CK(hipMemcpy(vq.data(), dq, nv * 4, hipMemcpyDeviceToHost));
        CK(hipFree(dcs));
        CK(hipFree(dout));
        CK(hipFree(don));
        CK(hipFree(dc));
        CK(hipFree(dq));
    }
    const double fast_s = seconds_since(t_fast);

    const auto t_ref = std::chrono::steady_clock::now();
    Tally t[2];
    uint64_t steps_applied = 0, steps_bad = 0;
    int shown = 0;
    for (uint32_t i = 0; i < n; ++i) {
        for (int mode = 0; mode < 2; ++mode) check_run(cs[i], mode, out[i].run[mode], t[mode], shown);
        steps_applied += out[i].m != 0u;
        if (!check_steps(cs[i], out[i])) {
            ++steps_bad;
            if (shown < 5) {
                ++shown;
                print_case("crawl_steps", cs[i], 0, nullptr, nullptr);
                fprintf(stderr, "  m %u delta (%a, %a, %a)\n", out[i].m, out[i].dl[0], out[i].dl[1], out[i].dl[2]);
            }
        }
    }
    const double ref_s = seconds_since(t_ref);

    uint64_t v_wrong[3] = {0, 0, 0}, v_amb[3] = {0, 0, 0};
    for (uint32_t i = 0; i < nv; ++i) {
        const int f = i < vx.n_random ? 0 : (i < vx.n_random + vx.n_integer ? 1 : 2);
        if (vq[i] == kAmbiguous) { ++v_amb[f]; continue; }
        if (vq[i] != vx.want[i] || (f == 2 && vx.on[i] != (float)vx.want[i])) {
            ++v_wrong[f];
            if (shown < 5) {
                ++shown;
                fprintf(stderr, "crawl_voxel: on %a c %a -> %d, voxel %d\n", vx.on[i], vx.c[i], vq[i], vx.want[i]);
            }
        }
    }

    bool ok = steps_bad == 0 && steps_applied > 0;
    for (int mode = 0; mode < 2; ++mode) {
        const Tally& m = t[mode];
        ok = ok && m.over_room == 0 && m.bad_prefix == 0 && m.incomplete == 0;
        ok = ok && m.capped * 100u <= m.runs;                    // <= 1 %
        ok = ok && m.zero * 100u <= m.runs * 30u;                // <= 30 %
        ok = ok && m.self_end * 100u >= m.runs * 20u;            // >= 20 %
        ok = ok && m.long_runs > 0 && m.long_fast * 100u >= m.long_runs * 95u;
    }
    ok = ok && v_wrong[0] + v_wrong[1] + v_wrong[2] == 0 && v_amb[0] < 50 && v_amb[2] == 0;

    printf("{\"mode\": \"%s\", \"cases\": %u", cpu ? "cpu" : "device", n);
    for (int mode = 0; mode < 2; ++mode) {
        const Tally& m = t[mode];
        printf(", \"%s\": {\"runs\": %llu, \"over_room\": %llu, \"bad_prefix\": %llu, \"incomplete\": %llu, "
               "\"capped\": %llu, \"capped_share\": %.5f, \"zero_share\": %.4f, \"self_end_share\": %.4f, "
               "\"long_runs\": %llu, \"long_fast\": %llu, \"trip_ratio\": %.5f, \"ref_iterations\": %llu}",
               mode ? "cluster_bits" : "plain", (unsigned long long)m.runs, (unsigned long long)m.over_room,
               (unsigned long long)m.bad_prefix, (unsigned long long)m.incomplete, (unsigned long long)m.capped,
               (double)m.capped / (double)m.runs, (double)m.zero / (double)m.runs, (double)m.self_end / (double)m.runs,
               (unsigned long long)m.long_runs, (unsigned long long)m.long_fast,
               m.long_runs ? (double)m.long_fast / (double)m.long_runs : 0.0, (unsigned long long)m.ref_iters);
    }
    printf(", \"steps\": {\"applied\": %llu, \"bad\": %llu}", (unsigned long long)steps_applied,
           (unsigned long long)steps_bad);
    printf(", \"voxel\": {\"random\": %zu, \"random_wrong\": %llu, \"random_ambiguous\": %llu, \"integer\": %zu, "
           "\"integer_wrong\": %llu, \"integer_ambiguous\": %llu, \"pinned\": %zu, \"pinned_wrong\": %llu, "
           "\"pinned_ambiguous\": %llu}",
           vx.n_random, (unsigned long long)v_wrong[0], (unsigned long long)v_amb[0], vx.n_integer,
           (unsigned long long)v_wrong[1], (unsigned long long)v_amb[1], vx.n_pinned, (unsigned long long)v_wrong[2],
           (unsigned long long)v_amb[2]);
    printf(", \"fast_s\": %.3f, \"ref_s\": %.3f, \"ok\": %s}\n", fast_s, ref_s, ok ? "true" : "false");
    return ok ? 0 : 1;
}
