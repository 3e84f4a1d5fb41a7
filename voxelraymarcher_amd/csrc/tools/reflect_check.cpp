// reflect_check -- vr_bounce_rays' and vr_shade_lights_reflect's arithmetic (vr_reflect_math.h) on a CPU.
//   reflect_check            mix_channel against the closed form -- the nearest integer to
//                            (A (255 - k) + B k) / 255, halves up -- for all 256^3 (A, B, k), its ends,
//                            and mix_rgb for packed words: every channel alone, among full channels and
//                            under set bits 24-31; the bounce's landmarks.  Returns 0, or prints the
//                            failing cases and returns 1.
//   reflect_check --bounce   reads from stdin a first line "TX TY TZ SCALE" (the translation's three
//                            floats as 8 hexadecimal digits each, the scale in decimal) and then one
//                            line per record pair "RAY HIT" (the 32 bytes of a vr_ray as 64 hexadecimal
//                            digits, the 64 bytes of a vr_hit as 128), and prints per pair the 32 bytes
//                            of the bounce ray as 64 digits: tests/test_reflect_check.py holds
//                            tests/reflect_ref.py to them.
#include "vr_reflect_math.h"

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

static void check_mix() {
    long cases = 0;
    for (uint32_t a = 0; a < 256u; ++a)
        for (uint32_t b = 0; b < 256u; ++b)
            for (uint32_t k = 0; k < 256u; ++k) {
                // round((a (255 - k) + b k) / 255), halves up, in 64 bits and without the function's form
                const unsigned long long twice = 2ull * ((unsigned long long)a * (255u - k) + (unsigned long long)b * k);
                unsigned long long want = twice / 510ull;
                if (twice - want * 510ull >= 255ull) ++want;
                const uint32_t got = vr::mix_channel(a, b, k);
                CHECK(got == want && got <= 255u, "mix_channel(%u, %u, %u) = %u, want %llu", a, b, k, got, want);
                // between its two ends
                CHECK(got >= (a < b ? a : b) && got <= (a < b ? b : a), "mix_channel(%u, %u, %u) = %u leaves [a, b]", a, b, k, got);
                ++cases;
            }
    CHECK(cases == 256L * 256L * 256L, "cases %ld", cases);
    for (uint32_t a = 0; a < 256u; ++a)
        for (uint32_t b = 0; b < 256u; ++b)
            CHECK(vr::mix_channel(a, b, 0) == a && vr::mix_channel(a, b, 255) == b && vr::mix_channel(a, a, b) == a,
                  "ends at (%u, %u)", a, b);
    // packed words: each channel alone, among full channels, and with bits 24-31 set in either word
    static const uint32_t kSome[] = {0, 1, 2, 63, 64, 96, 127, 128, 129, 200, 254, 255};
    for (uint32_t a : kSome)
        for (uint32_t b : kSome)
            for (uint32_t k = 0; k < 256u; ++k) {
                const uint32_t want = vr::mix_channel(a, b, k);
                for (int sh = 0; sh <= 16; sh += 8) {
                    const uint32_t hole = 0xFFFFFFFFu & ~(0xFFu << sh);
                    CHECK(vr::mix_rgb(a << sh, b << sh, k) == want << sh, "mix_rgb alone, (%u, %u, %u) at %d", a, b, k, sh);
                    const uint32_t got = vr::mix_rgb(hole | a << sh, hole | b << sh, k);
                    CHECK(((got >> sh) & 0xFFu) == want && (got >> 24) == 0u && (got | 0xFFu << sh) == 0x00FFFFFFu,
                          "mix_rgb among full channels, (%u, %u, %u) at %d: 0x%08X", a, b, k, sh, got);
                }
            }
    CHECK(vr::mix_rgb(0x123456u, 0xABCDEFu, 0) == 0x123456u && vr::mix_rgb(0x123456u, 0xABCDEFu, 255) == 0xABCDEFu,
          "k = 0 and k = 255");
    CHECK(vr::mix_rgb(0xFF123456u, 0xEEABCDEFu, 0) == 0x123456u && vr::mix_rgb(0xFF123456u, 0xEEABCDEFu, 255) == 0xABCDEFu,
          "bits 24-31 are dropped");
    CHECK(vr::mix_rgb(0x000000u, 0xFFFFFFu, 128) == 0x808080u && vr::mix_rgb(0xFF0000u, 0x0000FFu, 96) == 0x9F0060u, "landmarks");
}

static void check_bounce() {
    const float tr[3] = {1.5f, -2.25f, 0.125f}, point[3] = {3.5f, 63.75f, 0.0f};
    const int32_t region[3] = {2, -1, 0};
    const uint32_t dir[3] = {vr::reflect_bits(0.5f), vr::reflect_bits(-0.0f), vr::reflect_bits(3.0f)};
    uint32_t w[8];
    for (int a = 0; a < 3; ++a) {
        vr::bounce_ray(a, region, point, dir, tr, 4.0f, w);
        // (2 * 64 + 3.5) / 4 + 1.5, (-64 + 63.75) / 4 - 2.25, 0 / 4 + 0.125: all exact
        CHECK(w[0] == vr::reflect_bits(34.375f) && w[1] == vr::reflect_bits(-2.3125f) && w[2] == vr::reflect_bits(0.125f),
              "origin, axis %d", a);
        for (int c = 0; c < 3; ++c) CHECK(w[4 + c] == (dir[c] ^ (c == a ? 0x80000000u : 0u)), "direction %d, axis %d", c, a);
        CHECK(w[3] == 0u && w[7] == 0u, "reserved words, axis %d", a);
    }
    vr::bounce_ray(-1, region, point, dir, tr, 4.0f, w);
    for (int c = 0; c < 3; ++c) CHECK(w[c] == 0x7FC00000u && w[4 + c] == 0x7FC00000u, "no bounce: quiet NaNs");
    CHECK(w[3] == 0u && w[7] == 0u, "no bounce: reserved words");
    CHECK(vr::bounce_axis(1, 0, -1, 0) == 1 && vr::bounce_axis(1, 0, 0, 1) == 2 && vr::bounce_axis(1, -1, 0, 0) == 0, "axes");
    CHECK(vr::bounce_axis(0, 1, 0, 0) == -1 && vr::bounce_axis(2, 1, 0, 0) == -1 && vr::bounce_axis(3, 0, 0, 1) == -1 &&
              vr::bounce_axis(1, 0, 0, 0) == -1 && vr::bounce_axis(1, 1, 1, 0) == -1 && vr::bounce_axis(1, 0, 2, 0) == -1,
          "records without a bounce");
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

static int print_bounces() {
    unsigned t[3];
    unsigned long scale = 0;
    if (scanf("%8x %8x %8x %lu", &t[0], &t[1], &t[2], &scale) != 4) {
        fprintf(stderr, "--bounce: the first line is TX TY TZ SCALE\n");
        return 2;
    }
    float tr[3];
    for (int c = 0; c < 3; ++c) {
        const uint32_t u = (uint32_t)t[c];
        memcpy(&tr[c], &u, sizeof u);
    }
    const float scale_f = (float)(uint32_t)scale;
    char ray_s[80], hit_s[144];
    while (scanf("%79s %143s", ray_s, hit_s) == 2) {
        uint8_t ray_b[32], hit_b[64];
        if (!hex_bytes(ray_s, strlen(ray_s), ray_b, 32) || !hex_bytes(hit_s, strlen(hit_s), hit_b, 64)) {
            fprintf(stderr, "--bounce: a line is 64 hexadecimal digits, a blank, then 128\n");
            return 2;
        }
        // vr_ray: origin[3], reserved0, direction[3], reserved1; vr_hit: status, color, voxel[3], normal[3],
        // region[3], point[3], reserved[2] (little-endian words)
        uint32_t r[8], h[16], w[8];
        memcpy(r, ray_b, sizeof r);
        memcpy(h, hit_b, sizeof h);
        const int32_t region[3] = {(int32_t)h[8], (int32_t)h[9], (int32_t)h[10]};
        float point[3];
        memcpy(point, h + 11, sizeof point);
        vr::bounce_ray(vr::bounce_axis(h[0], (int32_t)h[5], (int32_t)h[6], (int32_t)h[7]), region, point, r + 4, tr, scale_f, w);
        uint8_t out[32];
        memcpy(out, w, sizeof out);
        for (int i = 0; i < 32; ++i) printf("%02x", out[i]);
        printf("\n");
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && strcmp(argv[1], "--bounce") == 0) return print_bounces();
    if (argc != 1) {
        fprintf(stderr, "usage: reflect_check [--bounce < records]\n");
        return 2;
    }
    check_mix();
    check_bounce();
    if (g_bad) printf("%d checks failed\n", g_bad);
    return g_bad ? 1 : 0;
}
