// Stand-alone host check of lsr::ring_mod_capacity_product (lsr_host_math.cpp), meant to be built with
// -fsanitize=address,undefined and run on a CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -Ilambda-snark-r_amd/csrc -Iinclude tools/capacity_product_check.cpp \
//       lambda-snark-r_amd/csrc/lsr_host_math.cpp lambda-snark-r_amd/csrc/lsr_keys.cpp -o capacity_product_check && ./capacity_product_check
// Over section 5p's grid of (n, q) and a grid of bound pairs that holds 0, 1, h = floor(q / 2) and h + 1 it asserts the zeros, the two
// identities with ring_mod_capacity_bounded and ring_mod_capacity, symmetry and monotonicity in each bound.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lsr_host_math.hpp"

#define CHECK(cond)                                                                                                            \
    do {                                                                                                                       \
        if (!(cond)) {                                                                                                         \
            std::fprintf(stderr, "FAILED %s at n = %u, q = %llu, bounds %llu, %llu\n", #cond, n, (unsigned long long)q,        \
                         (unsigned long long)ba, (unsigned long long)bb);                                                      \
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
            for (uint64_t ba : bounds)
                for (uint64_t bb : bounds) {
                    const size_t c = lsr::ring_mod_capacity_product(q, n, ba, bb);
                    ++calls;
                    nonzero += c != 0;
                    if (ba == 0 || bb == 0 || ba > h || bb > h || plain == 0) CHECK(c == 0);
                    else CHECK(c >= plain && c >= 1);
                    CHECK(c == lsr::ring_mod_capacity_product(q, n, bb, ba));
                    if (ba == h) CHECK(c == lsr::ring_mod_capacity_bounded(q, n, bb));
                    if (ba == h && bb == h) CHECK(c == plain);
                    // monotone: a smaller admissible bound never carries fewer products
                    for (uint64_t smaller : bounds)
                        if (smaller != 0 && smaller <= ba && ba <= h && c != 0) CHECK(lsr::ring_mod_capacity_product(q, n, smaller, bb) >= c);
                }
        }
    std::printf("ring_mod_capacity_product: %zu calls, %zu non-zero results: ok\n", calls, nonzero);
    return 0;
}
