// atmos_check -- vr_atmosphere_apply's and vr_shade_lights_atmosphere's arithmetic (vr_atmos_math.h) on a CPU.
//   atmos_check              lerp256's channel against the closed form -- the nearest integer to
//                            (A (256 - q) + B q) / 256, halves up -- for all 256 * 256 * 257 (A, B, q), its
//                            ends, and lerp256 for packed words: every channel alone, among full channels
//                            and under set bits 24-31; q256 at 0, subnormals, 1 - ulp, 1, NaN and the
//                            infinities; the colour bytes' landmarks; landmarks of the sky, the fog and
//                            the cases atmos leaves alone.  Returns 0, or prints the failing cases and
//                            returns 1.
//   atmos_check --atmos      reads from stdin a first line "TX TY TZ SCALE" (the translation's three
//                            floats as 8 hexadecimal digits each, the scale in decimal), a second line
//                            of the atmosphere's 17 floats in the order of vr_atmosphere (zenith, horizon,
//                            nadir, up, fog_color, fog_start, fog_end; 8 hexadecimal digits each) and its
//                            flags in decimal, and then one line per case "RAY HIT W" (the 32 bytes of a
//                            vr_ray as 64 hexadecimal digits, the 64 bytes of a vr_hit as 128, the colour
//                            word as 8), and prints per case atmos(W, RAY, HIT) as 8 hexadecimal digits:
//                            tests/test_atmos_check.py holds tests/atmos_ref.py to them.
#include "vr_atmos_math.h"

#include <initializer_list>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int g_bad = 0;
#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            if (++g_bad <= 20) {                  \
                printf("FAIL %s:%d: ", __FILE__, __LINE__); \
                printf(__VA_ARGS__);              \
                printf("  [%s]\n", #cond);        \
            }                                     \
        }                                         \
    } while (0)

static float from_bits(uint32_t u) {
    float f;
    memcpy(&f, &u, sizeof f);
    return f;
}

static void check_lerp() {
    long cases = 0;
    for (uint32_t a = 0; a < 256u; ++a)
        for (uint32_t b = 0; b < 256u; ++b)
            for (uint32_t q = 0; q <= 256u; ++q) {
                // round((a (256 - q) + b q) / 256), halves up, in 64 bits and without the function's form
                const unsigned long long twice = 2ull * ((unsigned long long)a * (256u - q) + (unsigned long long)b * q);
                unsigned long long want = twice / 512ull;
                if (twice - want * 512ull >= 256ull) ++want;
                const uint32_t got = vr::lerp256_channel(a, b, q);
                CHECK(got == want && got <= 255u, "lerp256_channel(%u, %u, %u) = %u, want %llu", a, b, q, got, want);
                CHECK(got >= (a < b ? a : b) && got <= (a < b ? b : a), "lerp256_channel(%u, %u, %u) = %u leaves [a, b]", a, b, q, got);
                ++cases;
            }
    CHECK(cases == 256L * 256L * 257L, "cases %ld", cases);
    for (uint32_t a = 0; a < 256u; ++a)
        for (uint32_t b = 0; b < 256u; ++b)
            CHECK(vr::lerp256_channel(a, b, 0) == a && vr::lerp256_channel(a, b, 256) == b && vr::lerp256_channel(a, a, b) == a,
                  "ends at (%u, %u)", a, b);
    static const uint32_t kSome[] = {0, 1, 2, 63, 64, 96, 127, 128, 129, 200, 254, 255};
    for (uint32_t a : kSome)
        for (uint32_t b : kSome)
            for (uint32_t q = 0; q <= 256u; ++q) {
                const uint32_t want = vr::lerp256_channel(a, b, q);
                for (int sh = 0; sh <= 16; sh += 8) {
                    const uint32_t hole = 0xFFFFFFFFu & ~(0xFFu << sh);
                    CHECK(vr::lerp256(a << sh, b << sh, q) == want << sh, "lerp256 alone, (%u, %u, %u) at %d", a, b, q, sh);
                    const uint32_t got = vr::lerp256(hole | a << sh, hole | b << sh, q);
                    CHECK(((got >> sh) & 0xFFu) == want && (got >> 24) == 0u && (got | 0xFFu << sh) == 0x00FFFFFFu,
                          "lerp256 among full channels, (%u, %u, %u) at %d: 0x%08X", a, b, q, sh, got);
                }
            }
    CHECK(vr::lerp256(0x123456u, 0xABCDEFu, 0) == 0x123456u && vr::lerp256(0x123456u, 0xABCDEFu, 256) == 0xABCDEFu, "q = 0 and q = 256");
    CHECK(vr::lerp256(0xFF123456u, 0xEEABCDEFu, 0) == 0x123456u && vr::lerp256(0xFF123456u, 0xEEABCDEFu, 256) == 0xABCDEFu,
          "bits 24-31 are dropped");
    // 255 * 128 / 256 = 127.5 -> 128; (255 * 160 + 0 * 96 + 128) >> 8 = 159, (0 * 160 + 255 * 96 + 128) >> 8 = 96
    CHECK(vr::lerp256(0x000000u, 0xFFFFFFu, 128) == 0x808080u && vr::lerp256(0xFF0000u, 0x0000FFu, 96) == 0x9F0060u, "landmarks");
}

static void check_q256() {
    const float nan = from_bits(0x7FC00000u), inf = from_bits(0x7F800000u);
    CHECK(vr::q256(0.0f) == 0u && vr::q256(-0.0f) == 0u, "zeros");
    CHECK(vr::q256(from_bits(1u)) == 0u && vr::q256(from_bits(0x007FFFFFu)) == 0u && vr::q256(from_bits(0x80000001u)) == 0u, "subnormals");
    CHECK(vr::q256(from_bits(0x3F7FFFFFu)) == 255u, "1 - ulp");
    CHECK(vr::q256(1.0f) == 256u && vr::q256(from_bits(0x3F800001u)) == 256u && vr::q256(3e38f) == 256u, "1 and above");
    CHECK(vr::q256(nan) == 0u && vr::q256(-nan) == 0u, "NaN");
    CHECK(vr::q256(inf) == 256u && vr::q256(-inf) == 0u, "infinities");
    CHECK(vr::q256(0.5f) == 128u && vr::q256(1.0f / 256.0f) == 1u && vr::q256(from_bits(0x3B7FFFFFu)) == 0u && vr::q256(-0.5f) == 0u,
          "inside");
    for (uint32_t q = 0; q < 256u; ++q) CHECK(vr::q256((float)q / 256.0f) == q, "q256(%u / 256)", q);
}

static void check_bytes() {
    const float nan = from_bits(0x7FC00000u), inf = from_bits(0x7F800000u);
    CHECK(vr::atmos_byte(0.0f) == 0u && vr::atmos_byte(-0.0f) == 0u && vr::atmos_byte(-1.0f) == 0u && vr::atmos_byte(-inf) == 0u, "not above 0");
    CHECK(vr::atmos_byte(nan) == 0u && vr::atmos_byte(-nan) == 0u, "NaN");
    CHECK(vr::atmos_byte(1.0f) == 255u && vr::atmos_byte(2.0f) == 255u && vr::atmos_byte(1e30f) == 255u && vr::atmos_byte(inf) == 255u, "1 and above");
    // 0.5 * 255 = 127.5, 0.25 * 255 = 63.75: truncated
    CHECK(vr::atmos_byte(0.5f) == 127u && vr::atmos_byte(0.25f) == 63u && vr::atmos_byte(from_bits(0x3F7FFFFFu)) == 254u, "truncation");
    CHECK(vr::atmos_byte(0.004f) == 1u &&vr::atmos_byte(0.003f) == 0u && vr::atmos_byte(from_bits(1u)) == 0u, "small values");
    const float c[3] = {1.0f, 0.5f, 0.25f};
    CHECK(vr::atmos_pack(c) == 0xFF7F3Fu, "packing: 0x%06X", vr::atmos_pack(c));
}

static void check_atmos() {
    const float zen[3] = {0.0f, 0.0f, 1.0f}, hor[3] = {1.0f, 1.0f, 1.0f}, nad[3] = {1.0f, 0.0f, 0.0f}, up[3] = {0.0f, 1.0f, 0.0f};
    const float fogc[3] = {0.5f, 0.5f, 0.5f};
    vr::AtmosParams p = vr::atmos_params(zen, hor, nad, up, fogc, 1.0f, 5.0f, 3u);
    CHECK(p.zenith == 0x0000FFu && p.horizon == 0xFFFFFFu && p.nadir == 0xFF0000u && p.fog == 0x7F7F7Fu && p.fog_span == 4.0f, "params");
    // straight up, straight down, level, half way up (d = (0, 3, 4) / any length: h = 0.6, q = 153)
    CHECK(vr::atmos_sky(p, 0.0f, 2.0f, 0.0f) == 0x0000FFu && vr::atmos_sky(p, 0.0f, -0.5f, 0.0f) == 0xFF0000u, "zenith and nadir");
    CHECK(vr::atmos_sky(p, 3.0f, 0.0f, -4.0f) == 0xFFFFFFu, "level");
    CHECK(vr::atmos_sky(p, 0.0f, 3.0f, 4.0f) == vr::lerp256(0xFFFFFFu, 0x0000FFu, 153u), "h = 0.6");
    CHECK(vr::atmos_sky(p, 0.0f, -3.0f, 4.0f) == vr::lerp256(0xFFFFFFu, 0xFF0000u, 153u), "h = -0.6");
    // a zero, an infinite and a NaN direction: h is NaN, the horizon
    const float nan = from_bits(0x7FC00000u), inf = from_bits(0x7F800000u);
    CHECK(vr::atmos_sky(p, 0.0f, 0.0f, 0.0f) == 0xFFFFFFu && vr::atmos_sky(p, 0.0f, inf, 0.0f) == 0xFFFFFFu &&
              vr::atmos_sky(p, nan, 1.0f, 0.0f) == 0xFFFFFFu, "NaN h gives the horizon");
    // the fog: region (1, 0, -1), point (0, 32, 64) at scale 16, translation (1, 2, 3): p = (5, 4, 3); from the
    // origin (5, 4, 0) D = 3, f = 0.5, q = 128
    const float tr[3] = {1.0f, 2.0f, 3.0f}, point[3] = {0.0f, 32.0f, 64.0f}, o[3] = {5.0f, 4.0f, 0.0f}, dir[3] = {0.0f, 3.0f, 4.0f};
    const int32_t region[3] = {1, 0, -1};
    CHECK(vr::atmos_fog(p, 0x102030u, o, region, point, tr, 16.0f) == vr::lerp256(0x102030u, 0x7F7F7Fu, 128u), "D = 3");
    const float o1[3] = {5.0f, 4.0f, 2.5f}, o2[3] = {5.0f, 4.0f, -2.0f}, o3[3] = {nan, 4.0f, 0.0f};
    CHECK(vr::atmos_fog(p, 0x102030u, o1, region, point, tr, 16.0f) == 0x102030u, "before fog_start");
    CHECK(vr::atmos_fog(p, 0x102030u, o2, region, point, tr, 16.0f) == 0x7F7F7Fu, "at fog_end");
    CHECK(vr::atmos_fog(p, 0xFF102030u, o3, region, point, tr, 16.0f) == 0x102030u, "a NaN distance: q = 0, bits 24-31 dropped");
    // atmos: by status and flags
    for (uint32_t flags = 0; flags < 4u; ++flags) {
        p.flags = flags;
        const uint32_t w = 0xAB102030u;
        CHECK(vr::atmos_word(p, w, 0u, o, dir, region, point, tr, 16.0f) == ((flags & 1u) ? vr::atmos_sky(p, 0.0f, 3.0f, 4.0f) : w), "MISS, flags %u", flags);
        CHECK(vr::atmos_word(p, w, 1u, o, dir, region, point, tr, 16.0f) == ((flags & 2u) ? vr::lerp256(w, 0x7F7F7Fu, 128u) : w), "VOXEL, flags %u", flags);
        for (uint32_t status : {2u, 3u, 4u, 0xFFFFFFFFu})
            CHECK(vr::atmos_word(p, w, status, o, dir, region, point, tr, 16.0f) == w, "status %u, flags %u", status, flags);
    }
    // fog_end <= fog_start: a step at fog_start (x / 0: +inf past it, -inf before it, NaN at it)
    p = vr::atmos_params(zen, hor, nad, up, fogc, 3.0f, 3.0f, 2u);
    CHECK(vr::atmos_fog(p, 0x102030u, o2, region, point, tr, 16.0f) == 0x7F7F7Fu && vr::atmos_fog(p, 0x102030u, o1, region, point, tr, 16.0f) == 0x102030u &&
              vr::atmos_fog(p, 0x102030u, o, region, point, tr, 16.0f) == 0x102030u, "a step");
}

static int hex_bytes(const char* s, size_t len, uint8_t* out, size_t n) {
    if (len != 2 * n) return 0;
    for (size_t i = 0; i < n; ++i) {
        unsigned v = 0;
        for (int k = 0; k < 2; ++k) {
            const char c = s[2 * i + k];
            const int d = c >= '0' && c <= '9' ? c - '0' : (c >= 'a' && c <= 'f' ? c - 'a' + 10 : (c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1));
            if (d < 0) return 0;
            v = v * 16u + (unsigned)d;
        }
        out[i] = (uint8_t)v;
    }
    return 1;
}

static int print_atmos() {
    unsigned t[3], a[17];
    unsigned long scale = 0, flags = 0;
    if (scanf("%8x %8x %8x %lu", &t[0], &t[1], &t[2], &scale) != 4) {
        fprintf(stderr, "--atmos: the first line is TX TY TZ SCALE\n");
        return 2;
    }
    for (int i = 0; i < 17; ++i)
        if (scanf("%8x", &a[i]) != 1) {
            fprintf(stderr, "--atmos: the second line is the atmosphere's 17 floats and its flags\n");
            return 2;
        }
    if (scanf("%lu", &flags) != 1) {
        fprintf(stderr, "--atmos: the second line is the atmosphere's 17 floats and its flags\n");
        return 2;
    }
    float tr[3], f[17];
    for (int c = 0; c < 3; ++c) tr[c] = from_bits((uint32_t)t[c]);
    for (int i = 0; i < 17; ++i) f[i] = from_bits((uint32_t)a[i]);
    const vr::AtmosParams p = vr::atmos_params(f, f + 3, f + 6, f + 9, f + 12, f[15], f[16], (uint32_t)flags);
    const float scale_f = (float)(uint32_t)scale;
    char ray_s[80], hit_s[144];
    unsigned w = 0;
    while (scanf("%79s %143s %8x", ray_s, hit_s, &w) == 3) {
        uint8_t ray_b[32], hit_b[64];
        if (!hex_bytes(ray_s, strlen(ray_s), ray_b, 32) || !hex_bytes(hit_s, strlen(hit_s), hit_b, 64)) {
            fprintf(stderr, "--atmos: a line is 64 hexadecimal digits, a blank, 128, a blank, then 8\n");
            return 2;
        }
        // vr_ray: origin[3], reserved0, direction[3], reserved1; vr_hit: status, color, voxel[3], normal[3],
        // region[3], point[3], reserved[2] (little-endian words)
        uint32_t h[16];
        float r[8], point[3];
        memcpy(r, ray_b, sizeof r);
        memcpy(h, hit_b, sizeof h);
        const int32_t region[3] = {(int32_t)h[8], (int32_t)h[9], (int32_t)h[10]};
        memcpy(point, h + 11, sizeof point);
        printf("%08x\n", vr::atmos_word(p, (uint32_t)w, h[0], r, r + 4, region, point, tr, scale_f));
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && strcmp(argv[1], "--atmos") == 0) return print_atmos();
    if (argc != 1) {
        fprintf(stderr, "usage: atmos_check [--atmos < cases]\n");
        return 2;
    }
    check_lerp();
    check_q256();
    check_bytes();
    check_atmos();
    if (g_bad) printf("%d checks failed\n", g_bad);
    return g_bad ? 1 : 0;
}
