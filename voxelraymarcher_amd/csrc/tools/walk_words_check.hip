// walk_words_check -- the small device forms every walk loop is built from (vr_device.h: f2i,
// f2u, lshl_or, bit_select, bit_sel, Ctx::cell, word_index, word_offset, word_bit5,
// word_bit5c) against plain C formulas computed here on the host.  One lane per case.  Built
// with the library's flags.  Prints one JSON line; exit 0 iff nothing differs, 1 otherwise
// (2: a HIP call failed).
//   walk_words_check [fractional cases] [seed]
//
//   cells   : all 64^3 integer cells (x, y, z) of a region, as floats: the in-loop conversion
//             (cell = the plain cast; f2i must agree), the mask word's index
//             y2 | x0..5 << 1 | y3..5 << 7 | z3..5 << 10, its byte offset base | index << 3 (and
//             << 2), and the voxel's bit (y & 3) << 3 | z & 7 in the low five bits;
//   frac    : the same for seeded positions in [0, 64), with +0, 63.999996 (the float below 64)
//             and positions next to every integer among them;
//   cvt     : f2i / f2u (truncate, saturate, NaN -> 0) at NaN, +-0, +-inf, +-2^31,
//             2^31 - 128, -2^31 - 256, denormals, +-63.5, 64.0 and seeded bit patterns;
//   select  : bit_select (asm) and bit_sel (C++) for masks 0 and ~0 over seeded bit patterns;
//   lshl_or : (a << s) | b for every shift the walks use (1, 3, 4, 10).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../vr_device.h"

namespace {

using F = vr::Ctx<vr::STORE_VCS, false, vr::kTileBudget>;

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
    std::fprintf(stderr, "walk_words_check: %s: %s\n", #x, hipGetErrorString(e_)); std::exit(2); } } while (0)

struct Pos { float x, y, z; uint32_t base; };
struct Words { int32_t c[3], f[3]; uint32_t wi, off3, off2, bit5, bit5c; };
struct Cvt { int32_t i; uint32_t u; };
struct Sel { uint32_t m, a, b; };
struct SelOut { uint32_t asm_form, c_form; };
struct Shl { uint32_t a, b; };
struct ShlOut { uint32_t s1, s3, s4, s10; };

// ---------------------------------------------------------------- code under test (device)
__global__ void k_words(const Pos* p, Words* w, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Pos q = p[i];
    Words r;
    r.c[0] = F::cell(q.x); r.c[1] = F::cell(q.y); r.c[2] = F::cell(q.z);
    r.f[0] = vr::f2i(q.x); r.f[1] = vr::f2i(q.y); r.f[2] = vr::f2i(q.z);
    const uint32_t x = (uint32_t)r.c[0], y = (uint32_t)r.c[1], z = (uint32_t)r.c[2];
    r.wi = F::word_index(x, y, z);
    r.off3 = F::word_offset<3u>(x, y, z, q.base);
    r.off2 = F::word_offset<2u>(x, y, z, q.base);
    r.bit5 = F::word_bit5(y, z);
    r.bit5c = F::word_bit5c(y, z);
    w[i] = r;
}
__global__ void k_cvt(const float* f, Cvt* o, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) o[i] = Cvt{vr::f2i(f[i]), vr::f2u(f[i])};
}
__global__ void k_sel(const Sel* s, SelOut* o, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float a = __uint_as_float(s[i].a), b = __uint_as_float(s[i].b);
    o[i] = SelOut{__float_as_uint(vr::bit_select(s[i].m, a, b)), __float_as_uint(vr::bit_sel(s[i].m, vr::walk_const(a), b))};
}
__global__ void k_shl(const Shl* s, ShlOut* o, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) o[i] = ShlOut{vr::lshl_or(s[i].a, 1u, s[i].b), vr::lshl_or(s[i].a, 3u, s[i].b), vr::lshl_or(s[i].a, 4u, s[i].b),
                            vr::lshl_or(s[i].a, 10u, s[i].b)};
}

// ---------------------------------------------------------------- the plain formulas (host)
int32_t ref_f2i(float f) {
    if (f != f) return 0;
    if (f >= 2147483648.0f) return INT32_MAX;
    if (f <= -2147483648.0f) return INT32_MIN;
    return (int32_t)std::trunc(f);
}
uint32_t ref_f2u(float f) {
    if (f != f) return 0u;
    if (f >= 4294967296.0f) return UINT32_MAX;
    if (f <= 0.0f) return 0u;
    return (uint32_t)std::trunc((double)f);
}
uint32_t ref_word(uint32_t x, uint32_t y, uint32_t z) {
    return ((y >> 2) & 1u) | (x << 1) | (((y >> 3) & 7u) << 7) | (((z >> 3) & 7u) << 10);
}

struct Rng {                         // splitmix64
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    uint32_t u32() { return (uint32_t)(next() >> 32); }
    float unit() { return (float)(next() >> 40) * (1.0f / 16777216.0f); }   // [0, 1)
};

template <class T>
T* to_device(const std::vector<T>& v) {
    T* d = nullptr;
    HIP_OK(hipMalloc(&d, v.size() * sizeof(T)));
    HIP_OK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return d;
}
template <class T>
std::vector<T> from_device(T* d, size_t n) {
    std::vector<T> v(n);
    HIP_OK(hipMemcpy(v.data(), d, n * sizeof(T), hipMemcpyDeviceToHost));
    HIP_OK(hipFree(d));
    return v;
}
template <class T>
T* device_out(size_t n) {
    T* d = nullptr;
    HIP_OK(hipMalloc(&d, n * sizeof(T)));
    HIP_OK(hipMemset(d, 0xA5, n * sizeof(T)));
    return d;
}
uint32_t grid(size_t n) { return (uint32_t)((n + 255) / 256); }

// positions -> mismatches
uint32_t check_words(const std::vector<Pos>& ps, const char* what) {
    Pos* dp = to_device(ps);
    Words* dw = device_out<Words>(ps.size());
    hipLaunchKernelGGL(k_words, dim3(grid(ps.size())), dim3(256), 0, 0, dp, dw, (uint32_t)ps.size());
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    const std::vector<Words> ws = from_device(dw, ps.size());
    HIP_OK(hipFree(dp));
    uint32_t bad = 0;
    for (size_t i = 0; i < ps.size(); ++i) {
        const Pos& p = ps[i];
        const Words& w = ws[i];
        const int32_t c[3] = {(int32_t)p.x, (int32_t)p.y, (int32_t)p.z};      // in [0, 64): the plain cast
        const uint32_t x = (uint32_t)c[0], y = (uint32_t)c[1], z = (uint32_t)c[2];
        const uint32_t wi = ref_word(x, y, z);
        const bool ok = w.c[0] == c[0] && w.c[1] == c[1] && w.c[2] == c[2] && w.f[0] == c[0] && w.f[1] == c[1] &&
                        w.f[2] == c[2] && wi < 8192u && w.wi == wi && w.off3 == (p.base | (wi << 3)) &&
                        w.off2 == (p.base | (wi << 2)) && (w.bit5 & 31u) == (((y & 3u) << 3) | (z & 7u)) &&
                        w.bit5c == ((y << 3) | (z & 7u)) && (w.bit5c & 31u) == (w.bit5 & 31u);
        if (!ok && bad++ < 5u)
            std::fprintf(stderr, "%s: (%a, %a, %a) base %#x: cell %d %d %d f2i %d %d %d word %#x off %#x %#x bit %#x %#x\n", what,
                         p.x, p.y, p.z, p.base, w.c[0], w.c[1], w.c[2], w.f[0], w.f[1], w.f[2], w.wi, w.off3, w.off2,
                         w.bit5, w.bit5c);
    }
    return bad;
}

}  // namespace

int main(int argc, char** argv) {
    const uint32_t n_frac = argc > 1 ? (uint32_t)std::strtoul(argv[1], nullptr, 0) : 200000u;
    Rng rng{argc > 2 ? std::strtoull(argv[2], nullptr, 0) : 20250607ull};

    // cells: every integer cell; base = a region's byte offset (region << 16), varied
    std::vector<Pos> cells;
    cells.reserve(64u * 64u * 64u);
    for (uint32_t x = 0; x < 64u; ++x)
        for (uint32_t y = 0; y < 64u; ++y)
            for (uint32_t z = 0; z < 64u; ++z) cells.push_back(Pos{(float)x, (float)y, (float)z, ((x * 64u + y) * 64u + z) % 4099u << 16});
    const uint32_t cells_bad = check_words(cells, "cells");

    // frac: seeded positions in [0, 64); the edge values take turns on every axis
    const float below64 = std::nextafterf(64.0f, 0.0f);                      // 63.999996
    std::vector<float> edge = {0.0f, below64, 0.5f, 0.99999994f, 1.0f, 63.0f, 63.5f, 1e-30f, 7.9999995f, 8.0f};
    for (int k = 1; k < 64; ++k) { edge.push_back(std::nextafterf((float)k, 0.0f)); edge.push_back(std::nextafterf((float)k, 64.0f)); }
    std::vector<Pos> frac;
    frac.reserve(n_frac + 3 * edge.size());
    for (size_t e = 0; e < edge.size(); ++e)
        for (int a = 0; a < 3; ++a) {
            float v[3] = {rng.unit() * 64.0f, rng.unit() * 64.0f, rng.unit() * 64.0f};
            v[a] = edge[e];
            v[(a + 1) % 3] = edge[(e * 7 + 3) % edge.size()];
            frac.push_back(Pos{v[0], v[1], v[2], (rng.u32() % 65536u) << 16});
        }
    while (frac.size() < n_frac + 3 * edge.size()) {
        float v[3];
        for (float& c : v) { c = rng.unit() * 64.0f; if (!(c < 64.0f)) c = below64; }
        frac.push_back(Pos{v[0], v[1], v[2], (rng.u32() % 65536u) << 16});
    }
    const uint32_t frac_bad = check_words(frac, "frac");

    // cvt
    std::vector<float> fs = {NAN, -NAN, 0.0f, -0.0f, INFINITY, -INFINITY, 2147483648.0f, -2147483648.0f, 2147483520.0f,
                             -2147483904.0f, 1e-45f, -1e-45f, 1e-39f, -1e-39f, 63.5f, -63.5f, 64.0f, 4294967296.0f,
                             4294967040.0f, 0.99999994f, -0.99999994f, 16777216.0f, 255.5f};
    const uint32_t cvt_named = (uint32_t)fs.size();
    for (uint32_t i = 0; i < 100000u; ++i) { const uint32_t b = rng.u32(); float f; std::memcpy(&f, &b, 4); fs.push_back(f); }
    uint32_t cvt_bad = 0;
    {
        float* df = to_device(fs);
        Cvt* dc = device_out<Cvt>(fs.size());
        hipLaunchKernelGGL(k_cvt, dim3(grid(fs.size())), dim3(256), 0, 0, df, dc, (uint32_t)fs.size());
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        const std::vector<Cvt> cs = from_device(dc, fs.size());
        HIP_OK(hipFree(df));
        for (size_t i = 0; i < fs.size(); ++i)
            if ((cs[i].i != ref_f2i(fs[i]) || cs[i].u != ref_f2u(fs[i])) && cvt_bad++ < 5u)
                std::fprintf(stderr, "cvt: %a: f2i %d (want %d) f2u %u (want %u)\n", fs[i], cs[i].i, ref_f2i(fs[i]), cs[i].u,
                             ref_f2u(fs[i]));
    }

    // select: masks 0 and ~0
    std::vector<Sel> ss;
    const float neg_eps = -vr::kEps;
    uint32_t ne;
    std::memcpy(&ne, &neg_eps, 4);
    for (uint32_t i = 0; i < 50000u; ++i) {
        const uint32_t a = (i & 1u) ? ne : rng.u32(), b = rng.u32();
        ss.push_back(Sel{0u, a, b});
        ss.push_back(Sel{~0u, a, b});
    }
    uint32_t sel_bad = 0;
    {
        Sel* ds = to_device(ss);
        SelOut* dout = device_out<SelOut>(ss.size());
        hipLaunchKernelGGL(k_sel, dim3(grid(ss.size())), dim3(256), 0, 0, ds, dout, (uint32_t)ss.size());
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        const std::vector<SelOut> os = from_device(dout, ss.size());
        HIP_OK(hipFree(ds));
        for (size_t i = 0; i < ss.size(); ++i) {
            const uint32_t want = ss[i].m ? ss[i].a : ss[i].b;
            if ((os[i].asm_form != want || os[i].c_form != want) && sel_bad++ < 5u)
                std::fprintf(stderr, "select: m %#x a %#x b %#x: %#x %#x\n", ss[i].m, ss[i].a, ss[i].b, os[i].asm_form, os[i].c_form);
        }
    }

    // lshl_or
    std::vector<Shl> hs;
    for (uint32_t i = 0; i < 50000u; ++i) hs.push_back(Shl{rng.u32() >> (i % 27u), rng.u32() >> (i % 31u)});
    uint32_t shl_bad = 0;
    {
        Shl* dh = to_device(hs);
        ShlOut* dout = device_out<ShlOut>(hs.size());
        hipLaunchKernelGGL(k_shl, dim3(grid(hs.size())), dim3(256), 0, 0, dh, dout, (uint32_t)hs.size());
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        const std::vector<ShlOut> os = from_device(dout, hs.size());
        HIP_OK(hipFree(dh));
        for (size_t i = 0; i < hs.size(); ++i) {
            const uint32_t a = hs[i].a, b = hs[i].b;
            const bool ok = os[i].s1 == ((a << 1) | b) && os[i].s3 == ((a << 3) | b) && os[i].s4 == ((a << 4) | b) &&
                            os[i].s10 == ((a << 10) | b);
            if (!ok && shl_bad++ < 5u) std::fprintf(stderr, "lshl_or: a %#x b %#x: %#x %#x %#x %#x\n", a, b, os[i].s1, os[i].s3, os[i].s4, os[i].s10);
        }
    }

    const bool ok = !cells_bad && !frac_bad && !cvt_bad && !sel_bad && !shl_bad;
    std::printf("{\"cells\": %zu, \"cells_bad\": %u, \"frac\": %zu, \"frac_edge\": %zu, \"frac_bad\": %u, \"cvt\": %zu, "
                "\"cvt_named\": %u, \"cvt_bad\": %u, \"select\": %zu, \"select_bad\": %u, \"lshl_or\": %zu, \"lshl_or_shifts\": 4, "
                "\"lshl_or_bad\": %u, \"ok\": %s}\n",
                cells.size(), cells_bad, frac.size(), 3 * edge.size(), frac_bad, fs.size(), cvt_named, cvt_bad, ss.size(), sel_bad,
                hs.size(), shl_bad, ok ? "true" : "false");
    return ok ? 0 : 1;
}
