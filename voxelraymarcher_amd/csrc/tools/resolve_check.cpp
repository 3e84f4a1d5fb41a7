// resolve_check -- vr_resolve's arithmetic (vr_resolve_math.h) on a CPU.
//   resolve_check                    the mean, exhaustively: for N = 1, 4, 16, 64 every channel sum
//                                    0 .. 255 * N against (sum + N / 2) / N, alone (resolve_mean)
//                                    and in each channel of resolve_pack while the other two
//                                    channels hold 0, their largest sum and a middle one (no carry
//                                    crosses a channel); resolve_add drops bits 24-31 and a block of
//                                    0xFFFFFFFF words resolves to 0xFFFFFF.  Returns 0, or prints the
//                                    failing cases and returns 1.
//   resolve_check --frame SEED W H S resolves the seeded fine frame of (S * W) x (S * H) words --
//                                    word k is the high half of x_k+1, x_0 = SEED, x_k+1 = x_k *
//                                    6364136223846793005 + 1442695040888963407 mod 2^64 -- with
//                                    resolve_block and prints the W * H words, one per line as eight
//                                    hexadecimal digits (tests/test_resolve_check.py holds them to
//                                    tests/aa_ref.py).
#include "vr_resolve_math.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

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

template <int S>
static long check_mean() {
    const uint32_t N = S * S, shift = vr::ResolveShift<S>::value, top = 255u * N;
    CHECK((1u << shift) == N, "S=%d\n", S);
    long cases = 0;
    const uint32_t others[3] = {0u, top, top / 3u};
    for (uint32_t sum = 0; sum <= top; ++sum) {
        const uint32_t want = (sum + N / 2u) / N;
        CHECK(vr::resolve_mean(sum, shift) == want, "S=%d sum=%u\n", S, sum);
        CHECK(want <= 255u, "S=%d sum=%u\n", S, sum);
        for (const uint32_t o : others) {
            const uint32_t wo = (o + N / 2u) / N;
            const vr::ResolveSum r = {sum << 16 | o, o}, g = {o << 16 | o, sum}, b = {o << 16 | sum, o};
            CHECK(vr::resolve_pack(r, shift) == (want << 16 | wo << 8 | wo), "S=%d red sum=%u other=%u\n", S, sum, o);
            CHECK(vr::resolve_pack(g, shift) == (wo << 16 | want << 8 | wo), "S=%d green sum=%u other=%u\n", S, sum, o);
            CHECK(vr::resolve_pack(b, shift) == (wo << 16 | wo << 8 | want), "S=%d blue sum=%u other=%u\n", S, sum, o);
            cases += 3;
        }
    }
    // a block of the largest words: every channel sums to 255 * N, bits 24-31 are dropped
    std::vector<uint32_t> full((size_t)S * S, 0xFFFFFFFFu);
    CHECK(vr::resolve_block<S>(full.data(), S) == 0x00FFFFFFu, "S=%d\n", S);
    vr::ResolveSum a = {0u, 0u};
    for (uint32_t k = 0; k < N; ++k) vr::resolve_add(a, 0xFF000000u | (k & 1u ? 0x00FF00FFu : 0x0000FF00u));
    CHECK(a.rb == (N / 2u * 255u) * 0x00010001u && a.g == (N - N / 2u) * 255u, "S=%d rb=%08X g=%08X\n", S, a.rb, a.g);
    return cases;
}

template <int S>
static void print_frame(const std::vector<uint32_t>& fine, uint32_t W, uint32_t H) {
    const size_t pitch = (size_t)S * W;
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x)
            printf("%08X\n", vr::resolve_block<S>(fine.data() + (size_t)y * S * pitch + (size_t)x * S, pitch));
}

int main(int argc, char** argv) {
    if (argc >= 2 && strcmp(argv[1], "--frame") == 0) {
        if (argc != 6) return 2;
        char* end = nullptr;
        unsigned long long v[4];
        for (int i = 0; i < 4; ++i) {
            v[i] = strtoull(argv[2 + i], &end, 0);
            if (end == argv[2 + i] || *end) return 2;
        }
        const uint32_t W = (uint32_t)v[1], H = (uint32_t)v[2], S = (uint32_t)v[3];
        if (v[1] < 1 || v[1] > 4096 || v[2] < 1 || v[2] > 4096 || (S != 1 && S != 2 && S != 4 && S != 8)) return 2;
        std::vector<uint32_t> fine((size_t)S * W * S * H);
        uint64_t x = v[0];
        for (uint32_t& w : fine) {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            w = (uint32_t)(x >> 32);
        }
        if (S == 1) print_frame<1>(fine, W, H);
        else if (S == 2) print_frame<2>(fine, W, H);
        else if (S == 4) print_frame<4>(fine, W, H);
        else print_frame<8>(fine, W, H);
        return 0;
    }
    if (argc != 1) return 2;
    const long cases = check_mean<1>() + check_mean<2>() + check_mean<4>() + check_mean<8>();
    if (g_bad) {
        printf("resolve_check: %d failures\n", g_bad);
        return 1;
    }
    printf("resolve_check OK: %ld packed cases, every channel sum of N = 1, 4, 16, 64\n", cases);
    return 0;
}
