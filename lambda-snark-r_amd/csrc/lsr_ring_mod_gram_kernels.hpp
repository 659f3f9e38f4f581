// The kernels of the Gram matrices of bounded ring vectors under an arbitrary modulus q (lsr_ring_mod_gram.hip, batch.h "Gram matrices
// under any modulus"), around launch_ntt on the handle's two prime contexts:
//   ring_mod_gram_lift_kernel     one read of every operand word: its centred representative as the canonical residue mod p1 and mod p2
//                                 into the two halves of the handle's Gram workspace, and "over the bound" / ">= q" folded into one
//                                 flag word per family.  Grid: x = runs of a vector's words (grid-stride), y = vectors, z = families —
//                                 every stride is a scalar offset, no lane divides.  16 bytes per lane and access where the source is
//                                 16-byte aligned (the workspace always is; every run and stride is a multiple of n >= 2 words).
//                                 CHECK: fold the flags (a wave ORs its lanes' bits first, then at most one atomic OR per wave);
//                                 STORE: write the residues.  A family taken in several column groups is checked whole by a pass
//                                 without STORE before its first group, so that its flags are complete before any reduce reads them.
//   ring_mod_gram_kernel          ring_gram_block (lsr_ring_gram_kernels.hpp) with the prime as the low bit of grid y: one launch for
//                                 both primes.  ModParams come as a two-element argument, indexed by that (wave-uniform) bit or
//                                 selected by a uniform branch on it; the a-hat / b-hat / g-hat of prime 1 lie `half` words behind those of prime 0.  (The host
//                                 launches the single-prime kernel per prime where this one is a wave short: kModGramBothPrimes.)
//   ring_mod_gram_reduce_kernel   ring_mod_reduce_kernel with the family as grid y: the word mod q of the integer a pair of residues
//                                 determines (ACC: added to what g holds), or 0 — whatever ACC says — where the family's flags are
//                                 set; lane 0 of a family's first workgroup writes status[family].
#pragma once

#include "lsr_ring_gram_kernels.hpp"
#include "lsr_ring_mod_kernels.hpp"

namespace lsr {

constexpr uint32_t kGramFlagOverBound = 1u, kGramFlagNotBelowQ = 2u;

struct GramLiftShape {
    size_t run;                 // words of one vector taken by this launch (columns n): even
    size_t src_vec, src_fam;    // words between consecutive vectors / families of the operand
    size_t dst_vec, dst_fam;    // the same in a prime's half of the workspace
    size_t half;                // words between the two halves
    uint64_t q, bound;          // a word x < q passes when its centred magnitude min(x, q - x) <= bound
};

template <bool VEC, bool CHECK, bool STORE>
__global__ void __launch_bounds__(kRingModThreads) ring_mod_gram_lift_kernel(uint64_t* __restrict__ dst, const uint64_t* __restrict__ x,
                                                                              uint32_t* __restrict__ flags, GramLiftShape s, LiftSource l0,
                                                                              LiftSource l1) {
    const size_t stride = (size_t)gridDim.x * kRingModThreads, first = (size_t)blockIdx.x * kRingModThreads + threadIdx.x;
    const uint64_t* const src = x + blockIdx.z * s.src_fam + blockIdx.y * s.src_vec;
    uint64_t* const d0 = dst + blockIdx.z * s.dst_fam + blockIdx.y * s.dst_vec;
    uint64_t* const d1 = d0 + s.half;
    uint32_t bits = 0;
    auto check = [&](uint64_t w) {
        if constexpr (CHECK) {
            const uint64_t mag = w <= l0.half ? w : s.q - w;
            bits |= w >= s.q ? kGramFlagNotBelowQ : (mag > s.bound ? kGramFlagOverBound : 0u);
        }
    };
    if constexpr (VEC) {
        const size_t pairs = s.run >> 1;
        for (size_t e = first; e < pairs; e += stride) {
            const ulonglong2 v = reinterpret_cast<const ulonglong2*>(src)[e];
            check(v.x);
            check(v.y);
            if constexpr (STORE) {
                reinterpret_cast<ulonglong2*>(d0)[e] = make_ulonglong2(l0.word(v.x), l0.word(v.y));
                reinterpret_cast<ulonglong2*>(d1)[e] = make_ulonglong2(l1.word(v.x), l1.word(v.y));
            }
        }
    } else {
        for (size_t e = first; e < s.run; e += stride) {
            const uint64_t w = src[e];
            check(w);
            if constexpr (STORE) {
                d0[e] = l0.word(w);
                d1[e] = l1.word(w);
            }
        }
    }
    if constexpr (CHECK) {
        // every lane of the workgroup arrives here: the ballots see whole waves
        const uint32_t wave_bits = (__ballot(bits & kGramFlagOverBound) ? kGramFlagOverBound : 0u) | (__ballot(bits & kGramFlagNotBelowQ) ? kGramFlagNotBelowQ : 0u);
        if (wave_bits && (threadIdx.x & (warpSize - 1)) == 0) atomicOr(&flags[blockIdx.z], wave_bits);
    }
}

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

// g: [families][words] (words even), r0 / r1: the families `r_fam` words apart
template <bool VEC, bool ACC>
__global__ void __launch_bounds__(kRingModThreads) ring_mod_gram_reduce_kernel(uint64_t* __restrict__ g, int32_t* __restrict__ status,
                                                                                const uint64_t* __restrict__ r0, const uint64_t* __restrict__ r1,
                                                                                const uint32_t* __restrict__ flags, size_t words, size_t r_fam,
                                                                                RingModConsts rc, ModParams p2, ModParams pq) {
    const size_t stride = (size_t)gridDim.x * kRingModThreads, first = (size_t)blockIdx.x * kRingModThreads + threadIdx.x;
    const uint32_t bits = flags[blockIdx.y];
    uint64_t* const out = g + blockIdx.y * words;
    const uint64_t* const a = r0 + blockIdx.y * r_fam;
    const uint64_t* const b = r1 + blockIdx.y * r_fam;
    if (first == 0) status[blockIdx.y] = (bits & kGramFlagNotBelowQ) ? -1 : (bits & kGramFlagOverBound) ? 0 : 1;
    if (bits) {
        if constexpr (VEC) {
            for (size_t e = first; e < (words >> 1); e += stride) reinterpret_cast<ulonglong2*>(out)[e] = make_ulonglong2(0, 0);
        } else {
            for (size_t e = first; e < words; e += stride) out[e] = 0;
        }
        return;
    }
    if constexpr (VEC) {
        for (size_t e = first; e < (words >> 1); e += stride) {
            const ulonglong2 x = reinterpret_cast<const ulonglong2*>(a)[e], y = reinterpret_cast<const ulonglong2*>(b)[e];
            ulonglong2 v;
            v.x = ring_mod_reduce_word(x.x, y.x, rc, p2, pq);
            v.y = ring_mod_reduce_word(x.y, y.y, rc, p2, pq);
            if constexpr (ACC) {
                const ulonglong2 old = reinterpret_cast<const ulonglong2*>(out)[e];
                v.x = ring_mod_add(old.x, v.x, pq.q);
                v.y = ring_mod_add(old.y, v.y, pq.q);
            }
            reinterpret_cast<ulonglong2*>(out)[e] = v;
        }
    } else {
        for (size_t e = first; e < words; e += stride) {
            const uint64_t v = ring_mod_reduce_word(a[e], b[e], rc, p2, pq);
            out[e] = ACC ? ring_mod_add(out[e], v, pq.q) : v;
        }
    }
}

}  // namespace lsr
