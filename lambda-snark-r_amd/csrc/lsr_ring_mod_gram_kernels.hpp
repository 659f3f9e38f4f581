// The kernel of the Gram matrices of bounded ring vectors under an arbitrary modulus q (lsr_ring_mod_gram.hip, batch.h "Gram matrices
// under any modulus"), between launch_ntt on the handle's two prime contexts; the checked lift before it and the gated
// reduce behind it are the ones every bounded call of a ring handle shares (lsr_ring_mod_kernels.hpp):
//   ring_mod_gram_kernel          ring_gram_block (lsr_ring_gram_kernels.hpp) with the prime as the low bit of grid y: one launch for
//                                 both primes.  ModParams come as a two-element argument, indexed by that (wave-uniform) bit or
//                                 selected by a uniform branch on it; the a-hat / b-hat / g-hat of prime 1 lie `half` words behind those of prime 0.  (The host
//                                 launches the single-prime kernel per prime where this one is a wave short: kModGramBothPrimes.)
#pragma once

#include "lsr_ring_gram_kernels.hpp"
#include "lsr_ring_mod_kernels.hpp"

namespace lsr {

struct GramModPrimes {
    ModParams p[2];
    size_t half;    // words between the two halves of the workspace
};

template <class A, int E, bool SYM, bool SYM2 = false>
__global__ void __launch_bounds__(kGramThreads) ring_mod_gram_kernel(uint64_t* __restrict__ g, const uint64_t* __restrict__ ahat,
                                                                       const uint64_t* __restrict__ bhat, GramShape s, GramModPrimes primes) {
    // The integer flavour selects the prime by a uniform branch: each side reads its ModParams from a fixed place of the kernel
    // arguments and the kernel needs 76 VGPRs where the indexed form (and the single-prime kernel) need 116.  The FP64 flavour indexes:
    // its branch form spills three SGPRs in the symmetrised mode.  (profiles/r34_ring_mod_gram_resource_usage.txt)
    if constexpr (std::is_same_v<A, ArithF64>) {
        const uint32_t i = blockIdx.y & 1u;
        const size_t off = i * primes.half;
        ring_gram_block<A, E, SYM, SYM2>(g + off, ahat + off, bhat + off, s, primes.p[i], blockIdx.y >> 1, blockIdx.z);
    } else if (blockIdx.y & 1u) {
        ring_gram_block<A, E, SYM, SYM2>(g + primes.half, ahat + primes.half, bhat + primes.half, s, primes.p[1], blockIdx.y >> 1, blockIdx.z);
    } else {
        ring_gram_block<A, E, SYM, SYM2>(g, ahat, bhat, s, primes.p[0], blockIdx.y >> 1, blockIdx.z);
    }
}

}  // namespace lsr
