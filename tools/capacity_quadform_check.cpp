// Stand-alone host check of lsr::ring_mod_capacity_quadform (lsr_host_math.cpp), meant to be built with
// -fsanitize=address,undefined and run on a CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -Ilambda-snark-r_amd/csrc -Iinclude tools/capacity_quadform_check.cpp \
//       lambda-snark-r_amd/csrc/lsr_host_math.cpp lambda-snark-r_amd/csrc/lsr_keys.cpp -o capacity_quadform_check && ./capacity_quadform_check
// Over section 5p's grid of (n, q) and a grid of bound pairs that holds 0, 1, h = floor(q / 2) and h + 1 it asserts the zeros, that a
// bound of 0 is h, monotonicity in each bound, and the exact identity with the bilinear capacity
//   capacity_quadform(q, n, g, c) == floor(capacity_product(q, n, g, c) / (n c))        wherever capacity_product is not saturated
// (both are nested floor divisions of (P - 1) / 2 by positive integers: n g c first, then n c), and <= it where it is.  The issue's
// table of values is pinned as well.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lsr_host_math.hpp"

#define CHECK(cond)                                                                                                            \
    do {                                                                                                                       \
        if (!(cond)) {                                                                                                         \
            std::fprintf(stderr, "FAILED %s at n = %u, q = %llu, bounds %llu, %llu\n", #cond, n, (unsigned long long)q,        \
                         (unsigned long long)bg, (unsigned long long)bc);                                                      \
            return 1;                                                                                                          \
        }                                                                                                                      \
    } while (0)

int main() {
    const std::vector<uint32_t> degrees = {0, 1, 2, 3, 8, 64, 256, 4096, 8192, 65536, 131072, 262144, 0xFFFFFFFFu};
    const std::vector<uint64_t> moduli = {0, 1, 2, 3, 3329, 1ull << 23, 4294967197ull, 1ull << 32, (1ull << 40) + 15, 8246337208321ull,
                                          (1ull << 44) + 1, 1ull << 63, ~0ull};
    size_t calls = 0, nonzero = 0;
    for (uint32_t n : degrees)
        for (uint64_t q : moduli) {
            const uint64_t h = q >> 1;
            std::vector<uint64_t> bounds = {0, 1, 2, 128, 1ull << 20, 1ull << 31, 1ull << 37, h, h + 1, ~0ull};
            const size_t plain = lsr::ring_mod_capacity(q, n);
            for (uint64_t bg : bounds)
                for (uint64_t bc : bounds) {
                    const size_t c = lsr::ring_mod_capacity_quadform(q, n, bg, bc);
                    ++calls;
                    nonzero += c != 0;
                    if (bg > h || bc > h || plain == 0) {
                        CHECK(c == 0);
                        continue;
                    }
                    // a bound of 0 states none, which is h
                    const uint64_t g = bg ? bg : h, cc = bc ? bc : h;
                    CHECK(c == lsr::ring_mod_capacity_quadform(q, n, g, cc));
                    // against the bilinear capacity: one more product with an operand within cc costs another n cc
                    const size_t bilinear = lsr::ring_mod_capacity_product(q, n, g, cc);
                    CHECK(bilinear >= 1);
                    if (bilinear != SIZE_MAX) CHECK(c == bilinear / n / cc);
                    else CHECK(c >= SIZE_MAX / n / cc);
                    // monotone: a smaller admissible bound never carries fewer products
                    for (uint64_t smaller : bounds)
                        if (smaller != 0 && smaller <= g) CHECK(lsr::ring_mod_capacity_quadform(q, n, smaller, bc) >= c);
                    for (uint64_t smaller : bounds)
                        if (smaller != 0 && smaller <= cc) CHECK(lsr::ring_mod_capacity_quadform(q, n, bg, smaller) >= c);
                }
        }
    struct Row {
        uint64_t q;
        uint32_t n;
        uint64_t bg, bc;
        size_t want;
    };
    const Row table[] = {{4294967197ull, 64, 0, 2, 4398042366208ull},
                         {4294967197ull, 64, 0, 1ull << 20, 15},
                         {4294967197ull, 64, 0, 1490944, 7},
                         {4294967197ull, 64, 0, 0, 0},
                         {(1ull << 40) + 15, 64, 0, 2, 17179852592ull},
                         {(1ull << 40) + 15, 64, 128, 2, SIZE_MAX},
                         {1ull << 32, 4096, 0, 2, 1073740786ull},
                         {1ull << 32, 4096, 0, 0, 0},
                         {1ull << 32, 65536, 0, 2, 4194301ull},
                         {3329, 256, 0, 0, 512471014808ull}};
    for (const Row& t : table) {
        const uint32_t n = t.n;
        const uint64_t q = t.q, bg = t.bg, bc = t.bc;
        CHECK(lsr::ring_mod_capacity_quadform(q, n, bg, bc) == t.want);
    }
    std::printf("ring_mod_capacity_quadform: %zu calls, %zu non-zero results: ok\n", calls, nonzero);
    return 0;
}
