// The kernels of the ring quadratic forms under an arbitrary modulus q (lsr_ring_mod_quadform.hip, batch.h "quadratic forms under any
// modulus"), between launch_ntt on the handle's two prime contexts and ring_mod_gram_reduce_kernel:
//   ring_mod_quadform_kernel        the row-wise evaluation of ring_quadform_kernel (lsr_ring_quadform_kernels.hpp)
//                                     Q-hat[k] = sum_i c-hat_i[k] * ( g-hat_ii[k] * c-hat_i[k] + w * sum_{l > i} g-hat_il[k] * c-hat_l[k] )
//                                   for BOTH primes in one launch: c-hat, g-hat and the destinations of prime 1 lie `half` words behind
//                                   those of prime 0, and w is the canonical residue of the centred offdiag mod each prime.
//   ring_mod_quadform_sum_kernel    adds the slices' partials in slice order, for both primes in one launch (grid z).
//   ring_mod_quadform_spread_kernel copies the flag word a shared c was checked into to the flag words of a chunk's families.
// Grid of the evaluation: x = runs of kQuadThreads positions, y = slices of the launch's packed pairs (and, where the prime is carried
// by the grid, the prime as the low bit), z = families of the chunk.  The launch covers the packed pairs [p_begin, p_end) of the
// triangle, g-hat holds them from p_begin on; slice y takes the pairs p_begin + [y count / slices, (y + 1) count / slices): balanced
// by PAIRS, so a slice may start and end inside a row.  The sum is linear in the pieces, every stored word is the canonical residue
// and residues are unique: the result does not depend on the slicing.  A launch's sums are complete — the groups of a family are
// joined mod q by the reduce pass, not in the evaluation domain — so nothing is carried in.  One slice: the canonical sum goes to
// sum[family][n].  More: to part[family][slice][n], and ring_mod_quadform_sum_kernel adds them.  No atomics, no LDS, no cross-lane
// traffic: a lane owns one evaluation position.  Plain 64-bit loads and stores.
// How the second prime is carried (CARRY), every way compiled for both flavours and chosen by the compiler's resource report
// (profiles/r37_ring_mod_quadform_resource_usage.txt, kModQuadCarry below):
//   kQuadCarryIndex    the low bit of grid y indexes a two-element ModParams argument;
//   kQuadCarryBranch   a uniform branch on that bit, each side reading its ModParams from a fixed place of the kernel arguments;
//   kQuadCarryLane     no grid bit: one lane evaluates its position under both primes, two independent dependency chains.
// Exactness per flavour is §5m's, which asks of the modulus only what p1, p2 < 2^44 give.  F64 — every mulmod_f64 has one canonical
// operand (c-hat_l, c-hat_i, w: words below the prime) and the other |x| < 2^50; the inner sum is re-centred every kRingDotF64Period
// products and before the outer multiplies, the outer sum every kRingDotF64Period rows and after the last one.  U64 — canonical
// products (Barrett) and canonical sums.
#pragma once

#include "lsr_ring_mod_kernels.hpp"
#include "lsr_ring_quadform_kernels.hpp"

namespace lsr {

constexpr int kQuadCarryIndex = 0, kQuadCarryBranch = 1, kQuadCarryLane = 2;

struct ModQuadShape {
    uint32_t logn, r;
    uint32_t p_begin, p_end;      // the packed pairs this launch covers; g-hat holds them from p_begin on
    uint32_t slices;
    size_t c_fam, g_fam;          // words between consecutive families of c-hat (0: one shared set) and of g-hat
    size_t half;                  // words between the two primes' halves of the workspace
};

struct ModQuadPrimes {
    ModParams p[2];
    uint64_t offdiag[2];          // the centred offdiag as a canonical word of each prime
};

// The pairs of slice `slice` of the launch for NP primes at once: prime k reads c-hat and g-hat at cp[k] / gp[k] (the family's, at
// this lane's position) and stores its canonical sum to to[k].
template <class A, int NP>
__device__ __forceinline__ void ring_mod_quadform_rows(uint64_t* const (&to)[NP], const uint64_t* const (&gp)[NP], const uint64_t* const (&cp)[NP],
                                                       const ModQuadShape& s, const ModParams* p, const uint64_t* offdiag, uint32_t slice) {
    using elem = typename A::elem;
    constexpr bool kF64 = std::is_same_v<A, ArithF64>;
    const size_t n = (size_t)1 << s.logn;
    // the pairs of this slice (uniform), and the row and column of the first one
    const uint32_t count = s.p_end - s.p_begin;
    const uint32_t p0 = s.p_begin + (uint32_t)((uint64_t)slice * count / s.slices);
    const uint32_t p1 = s.p_begin + (uint32_t)((uint64_t)(slice + 1) * count / s.slices);
    uint32_t i = 0, rest = p0;
    for (; i < s.r && rest >= s.r - i; ++i) rest -= s.r - i;     // (slices <= count: p0 is a pair of the triangle)
    uint32_t l = i + rest;

    size_t go = (size_t)(p0 - s.p_begin) << s.logn;
    elem off[NP], acc[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        off[k] = A::load(offdiag[k], p[k]);
        acc[k] = elem_from_bits<A>(0);
    }
    uint32_t rows = 0;
    for (uint32_t pp = p0; pp < p1; ++i, l = i) {
        const uint32_t row_end = min(p1, pp + (s.r - l));
        elem ci[NP], diag[NP], inner[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            ci[k] = A::load(cp[k][(size_t)i << s.logn], p[k]);
            diag[k] = elem_from_bits<A>(0);
            inner[k] = elem_from_bits<A>(0);
        }
        if (l == i) {
#pragma unroll
            for (int k = 0; k < NP; ++k) diag[k] = quad_product<A>(A::load(gp[k][go], p[k]), ci[k], p[k]);
            go += n, ++pp, ++l;
        }
#pragma unroll LSR_RING_QUADFORM_UNROLL
        for (uint32_t t = 0; pp < row_end; ++pp, ++l, ++t, go += n) {
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                inner[k] = ring_accumulate<A>(inner[k], quad_product<A>(A::load(gp[k][go], p[k]), A::load(cp[k][(size_t)l << s.logn], p[k]), p[k]), p[k]);
                if constexpr (kF64) {
                    if ((t & (kRingDotF64Period - 1u)) == kRingDotF64Period - 1u) inner[k] = recentre_f64(inner[k], p[k].qd, p[k].inv_qd);
                }
            }
        }
        ++rows;
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            if constexpr (kF64) inner[k] = recentre_f64(inner[k], p[k].qd, p[k].inv_qd);
            const elem u = ring_accumulate<A>(diag[k], quad_product<A>(inner[k], off[k], p[k]), p[k]);
            acc[k] = ring_accumulate<A>(acc[k], quad_product<A>(u, ci[k], p[k]), p[k]);
            if constexpr (kF64) {
                if ((rows & (kRingDotF64Period - 1u)) == 0) acc[k] = recentre_f64(acc[k], p[k].qd, p[k].inv_qd);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        if constexpr (kF64) acc[k] = recentre_f64(acc[k], p[k].qd, p[k].inv_qd);
        *to[k] = A::store_reduced(acc[k], p[k]);
    }
}

// one prime of the launch: `shift` is 0 or half
template <class A>
__device__ __forceinline__ void ring_mod_quadform_one(uint64_t* sum, uint64_t* part, const uint64_t* ghat, const uint64_t* chat, const ModQuadShape& s,
                                                      const ModParams& p, const uint64_t& offdiag, size_t shift, uint32_t slice, size_t pos) {
    const size_t n = (size_t)1 << s.logn;
    uint64_t* const to[1] = {(s.slices == 1 ? sum + blockIdx.z * n : part + ((size_t)blockIdx.z * s.slices + slice) * n) + shift + pos};
    const uint64_t* const gp[1] = {ghat + blockIdx.z * s.g_fam + shift + pos};
    const uint64_t* const cp[1] = {chat + blockIdx.z * s.c_fam + shift + pos};
    ring_mod_quadform_rows<A, 1>(to, gp, cp, s, &p, &offdiag, slice);
}

template <class A, int CARRY>
__global__ void __launch_bounds__(kQuadThreads) ring_mod_quadform_kernel(uint64_t* __restrict__ sum, uint64_t* __restrict__ part,
                                                                          const uint64_t* __restrict__ ghat, const uint64_t* __restrict__ chat,
                                                                          ModQuadShape s, ModQuadPrimes primes) {
    const size_t n = (size_t)1 << s.logn;
    const size_t pos = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= n) return;
    if constexpr (CARRY == kQuadCarryIndex) {
        const uint32_t i = blockIdx.y & 1u;                    // wave-uniform: kernel arguments at a scalar offset
        ring_mod_quadform_one<A>(sum, part, ghat, chat, s, primes.p[i], primes.offdiag[i], i * s.half, blockIdx.y >> 1, pos);
    } else if constexpr (CARRY == kQuadCarryBranch) {
        if (blockIdx.y & 1u) ring_mod_quadform_one<A>(sum, part, ghat, chat, s, primes.p[1], primes.offdiag[1], s.half, blockIdx.y >> 1, pos);
        else ring_mod_quadform_one<A>(sum, part, ghat, chat, s, primes.p[0], primes.offdiag[0], 0, blockIdx.y >> 1, pos);
    } else {
        uint64_t* const d0 = (s.slices == 1 ? sum + blockIdx.z * n : part + ((size_t)blockIdx.z * s.slices + blockIdx.y) * n) + pos;
        const uint64_t* const g0 = ghat + blockIdx.z * s.g_fam + pos;
        const uint64_t* const c0 = chat + blockIdx.z * s.c_fam + pos;
        uint64_t* const to[2] = {d0, d0 + s.half};
        const uint64_t* const gp[2] = {g0, g0 + s.half};
        const uint64_t* const cp[2] = {c0, c0 + s.half};
        ring_mod_quadform_rows<A, 2>(to, gp, cp, s, primes.p, primes.offdiag, blockIdx.y);
    }
}

// sum[prime][family] = part[prime][family][0] + ... + part[prime][family][slices - 1], canonical words in and out, in this order: one
// conditional subtraction per sum (the primes are below 2^44).  Grid: x = runs of positions, y = families, z = prime.
struct ModQuadSumShape {
    uint32_t logn, slices;
    size_t half;
    uint64_t p[2];
};

__global__ void __launch_bounds__(kQuadThreads) ring_mod_quadform_sum_kernel(uint64_t* __restrict__ sum, const uint64_t* __restrict__ part, ModQuadSumShape s) {
    const size_t n = (size_t)1 << s.logn;
    const size_t pos = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= n) return;
    const uint64_t q = s.p[blockIdx.z];
    const uint64_t* from = part + blockIdx.z * s.half + (size_t)blockIdx.y * s.slices * n + pos;
    uint64_t acc = 0;
    // (unrolled: the loads of eight slices are in flight together)
#pragma unroll 8
    for (uint32_t t = 0; t < s.slices; ++t, from += n) {
        acc += *from;
        acc = acc >= q ? acc - q : acc;
    }
    sum[blockIdx.z * s.half + blockIdx.y * n + pos] = acc;
}

// flags[j] = *shared for j < families: the flag words of a chunk start from what the check of a shared c found (the lifts of g then OR
// theirs in); runs in stream order between the lifts, so plain loads and stores do.
__global__ void __launch_bounds__(kRingModThreads) ring_mod_quadform_spread_kernel(uint32_t* __restrict__ flags, const uint32_t* __restrict__ shared,
                                                                                    uint32_t families) {
    const uint32_t j = blockIdx.x * kRingModThreads + threadIdx.x;
    if (j < families) flags[j] = *shared;
}

}  // namespace lsr
