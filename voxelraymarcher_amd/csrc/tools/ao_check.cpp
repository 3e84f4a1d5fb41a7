// ao_check -- vr_occlusion's arithmetic (vr_occlusion_math.h) on a CPU.
//   ao_check                   the corner rule for all 256 occupancy patterns against the table spelled
//                              out below; ao_acc, ao_round, ao_factor and scale_rgb against plain loops:
//                              every (q_u, q_w) of a coarse grid with the edges under every combination
//                              of four levels, every acc, every (ao, strength), every (byte, m).
//                              Returns 0, or prints the failing cases and returns 1.
//   ao_check --records R O ... (pairs: R the 64 bytes of a vr_hit record as 128 hexadecimal digits, O
//                              the occupancy pattern of its eight neighbours as two) prints per pair
//                              "axis q_u q_w ao" (axis -1 and q 0 0 for a record that is open by
//                              definition): tests/test_ao_check.py holds tests/ao_ref.py to them.
#include "vr_occlusion_math.h"

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

// L(-1,-1) | L(+1,-1) << 2 | L(-1,+1) << 4 | L(+1,+1) << 6 of occupancy pattern i, whose bit j is the
// cell (du, dw) = (-1,-1) (0,-1) (1,-1) (-1,0) (1,0) (-1,1) (0,1) (1,1) for j = 0..7
static const uint8_t kLevels[256] = {
    0xFF, 0xFE, 0xFA, 0xF9, 0xFB, 0xFA, 0xF6, 0xF5, 0xEE, 0xED, 0xE8, 0xE8, 0xEA, 0xE9, 0xE4, 0xE4,
    0xBB, 0xBA, 0xB2, 0xB1, 0xB7, 0xB6, 0xB2, 0xB1, 0xAA, 0xA9, 0xA0, 0xA0, 0xA6, 0xA5, 0xA0, 0xA0,
    0xEF, 0xEE, 0xEA, 0xE9, 0xEB, 0xEA, 0xE6, 0xE5, 0xDE, 0xDD, 0xD8, 0xD8, 0xDA, 0xD9, 0xD4, 0xD4,
    0xAB, 0xAA, 0xA2, 0xA1, 0xA7, 0xA6, 0xA2, 0xA1, 0x9A, 0x99, 0x90, 0x90, 0x96, 0x95, 0x90, 0x90,
    0xAF, 0xAE, 0xAA, 0xA9, 0xAB, 0xAA, 0xA6, 0xA5, 0x8E, 0x8D, 0x88, 0x88, 0x8A, 0x89, 0x84, 0x84,
    0x2B, 0x2A, 0x22, 0x21, 0x27, 0x26, 0x22, 0x21, 0x0A, 0x09, 0x00, 0x00, 0x06, 0x05, 0x00, 0x00,
    0x9F, 0x9E, 0x9A, 0x99, 0x9B, 0x9A, 0x96, 0x95, 0x8E, 0x8D, 0x88, 0x88, 0x8A, 0x89, 0x84, 0x84,
    0x1B, 0x1A, 0x12, 0x11, 0x17, 0x16, 0x12, 0x11, 0x0A, 0x09, 0x00, 0x00, 0x06, 0x05, 0x00, 0x00,
    0xBF, 0xBE, 0xBA, 0xB9, 0xBB, 0xBA, 0xB6, 0xB5, 0xAE, 0xAD, 0xA8, 0xA8, 0xAA, 0xA9, 0xA4, 0xA4,
    0x7B, 0x7A, 0x72, 0x71, 0x77, 0x76, 0x72, 0x71, 0x6A, 0x69, 0x60, 0x60, 0x66, 0x65, 0x60, 0x60,
    0xAF, 0xAE, 0xAA, 0xA9, 0xAB, 0xAA, 0xA6, 0xA5, 0x9E, 0x9D, 0x98, 0x98, 0x9A, 0x99, 0x94, 0x94,
    0x6B, 0x6A, 0x62, 0x61, 0x67, 0x66, 0x62, 0x61, 0x5A, 0x59, 0x50, 0x50, 0x56, 0x55, 0x50, 0x50,
    0x6F, 0x6E, 0x6A, 0x69, 0x6B, 0x6A, 0x66, 0x65, 0x4E, 0x4D, 0x48, 0x48, 0x4A, 0x49, 0x44, 0x44,
    0x2B, 0x2A, 0x22, 0x21, 0x27, 0x26, 0x22, 0x21, 0x0A, 0x09, 0x00, 0x00, 0x06, 0x05, 0x00, 0x00,
    0x5F, 0x5E, 0x5A, 0x59, 0x5B, 0x5A, 0x56, 0x55, 0x4E, 0x4D, 0x48, 0x48, 0x4A, 0x49, 0x44, 0x44,
    0x1B, 0x1A, 0x12, 0x11, 0x17, 0x16, 0x12, 0x11, 0x0A, 0x09, 0x00, 0x00, 0x06, 0x05, 0x00, 0x00,
};

static void check_corners() {
    static const int du[8] = {-1, 0, 1, -1, 1, -1, 0, 1}, dw[8] = {-1, -1, -1, 0, 0, 1, 1, 1};
    for (int j = 0; j < 8; ++j) CHECK(vr::ao_du(j) == du[j] && vr::ao_dw(j) == dw[j], "cell %d", j);
    for (uint32_t occ = 0; occ < 256u; ++occ)
        CHECK(vr::ao_levels(occ) == kLevels[occ], "pattern 0x%02X: 0x%02X, table 0x%02X", occ, vr::ao_levels(occ), kLevels[occ]);
    // the table's own landmarks: nothing stored is open, both sides stored close a corner whatever
    // the corner cell, a lone corner cell costs one level, a lone side one level at two corners
    CHECK(kLevels[0x00] == 0xFF && kLevels[0xFF] == 0x00 && kLevels[0x5A] == 0x00, "open, full, the four sides");
    CHECK(kLevels[0x01] == 0xFE && kLevels[0x80] == 0xBF && kLevels[0x02] == 0xFA && kLevels[0x0A] == 0xE8, "single cells");
    CHECK(vr::ao_corner(1, 1, 0) == 0 && vr::ao_corner(1, 0, 1) == 1 && vr::ao_corner(0, 0, 1) == 2 && vr::ao_corner(0, 0, 0) == 3,
          "the rule");
    for (int a = 0; a < 3; ++a) CHECK(vr::ao_axis_u(a) == (a + 1) % 3 && vr::ao_axis_w(a) == (a + 2) % 3, "tangent axes of %d", a);
    CHECK(vr::ao_axis(1, 0, 0) == 0 && vr::ao_axis(0, -1, 0) == 1 && vr::ao_axis(0, 0, 1) == 2, "unit normals");
    CHECK(vr::ao_axis(0, 0, 0) == -1 && vr::ao_axis(1, 1, 0) == -1 && vr::ao_axis(0, 2, 0) == -1 && vr::ao_axis(1, 0, -1) == -1 &&
              vr::ao_axis(-1, 0, 2) == -1, "normals that are none");
}

static void check_sums() {
    static const uint32_t kGrid[] = {0, 1, 2, 17, 64, 127, 128, 129, 200, 254, 255, 256};
    long cases = 0;
    for (uint32_t lv = 0; lv < 256u; ++lv)
        for (uint32_t qu : kGrid)
            for (uint32_t qw : kGrid) {
                // the definition: the four corners weighted by the opposite areas, summed in 64 bits
                unsigned long long want = 0;
                for (int k = 0; k < 4; ++k) {
                    const unsigned long long wu = (k & 1) ? qu : 256u - qu, ww = (k & 2) ? qw : 256u - qw;
                    want += wu * ww * ((lv >> (2 * k)) & 3u);
                }
                const uint32_t got = vr::ao_acc(lv, qu, qw);
                CHECK(got == want && got <= 196608u, "ao_acc(0x%02X, %u, %u) = %u, want %llu", lv, qu, qw, got, want);
                ++cases;
            }
    CHECK(cases == 256L * 144L, "cases %ld", cases);
    CHECK(vr::ao_acc(0xFF, 100, 37) == 196608u && vr::ao_acc(0xFD, 0, 0) == 65536u && vr::ao_acc(0x7F, 256, 256) == 65536u,
          "corners at the edges");
    // ao_round: the nearest of 0..255 to acc * 255 / 196608, halves up; monotonic
    uint32_t prev = 0;
    for (uint32_t acc = 0; acc <= 196608u; ++acc) {
        const uint32_t got = vr::ao_round(acc);
        const unsigned long long twice = 2ull * acc * 255ull;          // 2 * the exact value * 196608
        unsigned long long want = twice / (2ull * 196608ull);
        if (twice - want * 2ull * 196608ull >= 196608ull) ++want;
        CHECK(got == want && got >= prev && got <= 255u, "ao_round(%u) = %u, want %llu", acc, got, want);
        prev = got;
    }
    CHECK(vr::ao_round(0) == 0 && vr::ao_round(196608u) == 255u && vr::ao_value(0x00, 3, 250) == 255u &&
              vr::ao_value(0xFF, 128, 128) == 0u, "the ends");
    // ao_factor
    for (uint32_t ao = 0; ao < 256u; ++ao)
        for (uint32_t st = 0; st < 256u; ++st) {
            uint32_t drop = 0;                                         // round((255 - ao) * st / 255), halves up
            while ((drop + 1u) * 510u <= 2u * (255u - ao) * st + 255u) ++drop;
            CHECK(vr::ao_factor(ao, st) == 255u - drop, "ao_factor(%u, %u) = %u, want %u", ao, st, vr::ao_factor(ao, st), 255u - drop);
        }
    for (uint32_t x = 0; x < 256u; ++x)
        CHECK(vr::ao_factor(x, 0) == 255u && vr::ao_factor(x, 255) == x && vr::ao_factor(255, x) == 255u, "factor ends at %u", x);
    // scale_rgb: every (byte, m) in every channel, under two fillings of the others and the top byte
    for (uint32_t b = 0; b < 256u; ++b)
        for (uint32_t m = 0; m < 256u; ++m) {
            uint32_t want = 0;                                         // round(b * m / 255), halves up
            while ((want + 1u) * 510u <= 2u * b * m + 255u) ++want;
            for (int sh = 0; sh <= 16; sh += 8) {
                const uint32_t got = vr::scale_rgb(b << sh, m), got2 = vr::scale_rgb((0xFFFFFFFFu & ~(0xFFu << sh)) | b << sh, m);
                CHECK(got == want << sh, "scale_rgb(0x%08X, %u) = 0x%08X", b << sh, m, got);
                CHECK(((got2 >> sh) & 0xFFu) == want && (got2 >> 24) == 0u, "scale_rgb among full channels, %u * %u at %d", b, m, sh);
            }
        }
    CHECK(vr::scale_rgb(0xAB123456u, 255) == 0x123456u && vr::scale_rgb(0x123456u, 0) == 0u, "m = 255 and m = 0");
}

static int hex_bytes(const char* s, uint8_t* out, size_t n) {
    if (strlen(s) != 2 * n) return 0;
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

static int print_records(int n, char** args) {
    for (int i = 0; i + 1 < n; i += 2) {
        uint8_t raw[64], occ = 0;
        if (!hex_bytes(args[i], raw, 64) || !hex_bytes(args[i + 1], &occ, 1)) {
            fprintf(stderr, "--records needs pairs: 128 hexadecimal digits, then two\n");
            return 2;
        }
        // vr_hit: status, color, voxel[3], normal[3], region[3], point[3], reserved[2] (little-endian words)
        uint32_t w[16];
        memcpy(w, raw, sizeof w);
        float pt[3];
        memcpy(pt, w + 11, sizeof pt);
        const int a = vr::ao_axis((int32_t)w[5], (int32_t)w[6], (int32_t)w[7]);
        if (w[0] != 1u || a < 0) {
            printf("-1 0 0 %u\n", vr::kAoOpen);
            continue;
        }
        const int u = vr::ao_axis_u(a), t = vr::ao_axis_w(a);
        const uint32_t qu = vr::ao_q(pt[u], (int32_t)w[2 + u], (int32_t)w[8 + u]), qw = vr::ao_q(pt[t], (int32_t)w[2 + t], (int32_t)w[8 + t]);
        printf("%d %u %u %u\n", a, qu, qw, vr::ao_value(occ, qu, qw));
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 4 && argc % 2 == 0 && strcmp(argv[1], "--records") == 0) return print_records(argc - 2, argv + 2);
    if (argc != 1) {
        fprintf(stderr, "usage: ao_check [--records RECORD OCCUPANCY ...]\n");
        return 2;
    }
    check_corners();
    check_sums();
    if (g_bad) printf("%d checks failed\n", g_bad);
    return g_bad ? 1 : 0;
}
