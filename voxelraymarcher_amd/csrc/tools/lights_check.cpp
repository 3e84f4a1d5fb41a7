// lights_check -- vr_shade_lights' arithmetic (vr_lights_math.h) on a CPU.
//   lights_check                     sat_add_rgb against a plain per-channel loop: every pair of
//                                    values of each channel (256 x 256) under several fillings of
//                                    the other two channels, carries between channels, bits 24-31
//                                    dropped.  Returns 0, or prints the failing cases and returns 1.
//   lights_check --ambient A0 A1 A2  (the three ambient floats as hexadecimal bit patterns) prints,
//                                    for c = 0..255, "c word": ambient_term of the stored colour
//                                    c << 16 | c << 8 | c as eight hexadecimal digits
//                                    (tests/test_lights_check.py holds them to tests/lights_ref.py).
#include "vr_lights_math.h"

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

// the definition, channel by channel
static uint32_t plain(uint32_t a, uint32_t b) {
    uint32_t out = 0;
    for (int sh = 16; sh >= 0; sh -= 8) {
        const uint32_t sum = ((a >> sh) & 0xFFu) + ((b >> sh) & 0xFFu);
        out |= (sum < 255u ? sum : 255u) << sh;
    }
    return out;
}

static void check_sat_add() {
    // what the two other channels (and the top byte) hold while one channel runs through every sum
    static const uint32_t kFill[][2] = {{0x00000000u, 0x00000000u}, {0x00FFFFFFu, 0x00FFFFFFu}, {0x00FFFFFFu, 0x00000000u},
                                        {0x00808080u, 0x007F7F7Fu}, {0x00808080u, 0x00808080u}, {0xFFFFFFFFu, 0xFFFFFFFFu},
                                        {0xA5123456u, 0x5AFEDCBAu}};
    long cases = 0;
    for (int sh = 0; sh <= 16; sh += 8)
        for (const auto& f : kFill)
            for (uint32_t x = 0; x < 256u; ++x)
                for (uint32_t y = 0; y < 256u; ++y) {
                    const uint32_t keep = ~(0xFFu << sh);
                    const uint32_t a = (f[0] & keep) | x << sh, b = (f[1] & keep) | y << sh;
                    const uint32_t got = vr::sat_add_rgb(a, b), want = plain(a, b);
                    CHECK(got == want, "sat_add_rgb(0x%08X, 0x%08X) = 0x%08X, want 0x%08X", a, b, got, want);
                    CHECK(((got >> sh) & 0xFFu) == (x + y < 255u ? x + y : 255u), "channel at bit %d: %u + %u", sh, x, y);
                    ++cases;
                }
    CHECK(cases == 3L * 7L * 65536L, "cases %ld", cases);
    // no carry crosses a channel, in either direction
    CHECK(vr::sat_add_rgb(0x0000FFu, 0x000001u) == 0x0000FFu, "blue does not carry into green");
    CHECK(vr::sat_add_rgb(0x00FF00u, 0x000100u) == 0x00FF00u, "green does not carry into red");
    CHECK(vr::sat_add_rgb(0xFF0000u, 0x010000u) == 0xFF0000u, "red does not carry into bits 24-31");
    CHECK(vr::sat_add_rgb(0xFFFFFFu, 0xFFFFFFu) == 0xFFFFFFu, "all three clamp");
    CHECK(vr::sat_add_rgb(0x7F80FFu, 0x808000u) == 0xFFFFFFu, "sums of exactly 255 and 256");
    CHECK(vr::sat_add_rgb(0x010203u, 0x040506u) == 0x050709u, "a plain sum");
    // bits 24-31 of either word are dropped
    for (uint32_t top = 1; top < 256u; ++top) {
        CHECK(vr::sat_add_rgb(top << 24 | 0x102030u, 0x010101u) == 0x112131u, "top byte 0x%02X of a", top);
        CHECK(vr::sat_add_rgb(0x102030u, top << 24 | 0x010101u) == 0x112131u, "top byte 0x%02X of b", top);
        CHECK(vr::sat_add_rgb(top << 24, (256u - top) << 24) == 0u, "top bytes alone");
    }
    CHECK(vr::sat_add_rgb(0u, 0xFF123456u) == 0x123456u, "a term folded into 0 loses only its top byte");
}

static int print_ambient(char** bits) {
    float amb[3];
    for (int i = 0; i < 3; ++i) {
        char* end = nullptr;
        const unsigned long u = strtoul(bits[i], &end, 16);
        if (end == bits[i] || *end != '\0' || u > 0xFFFFFFFFul) {
            fprintf(stderr, "--ambient needs three floats as hexadecimal bit patterns\n");
            return 2;
        }
        const uint32_t w = (uint32_t)u;
        memcpy(&amb[i], &w, sizeof w);
    }
    for (uint32_t c = 0; c < 256u; ++c) printf("%u %08X\n", c, vr::ambient_term(c << 16 | c << 8 | c, amb));
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 5 && strcmp(argv[1], "--ambient") == 0) return print_ambient(argv + 2);
    if (argc != 1) {
        fprintf(stderr, "usage: lights_check [--ambient A0 A1 A2]\n");
        return 2;
    }
    check_sat_add();
    if (g_bad) printf("%d checks failed\n", g_bad);
    return g_bad ? 1 : 0;
}
