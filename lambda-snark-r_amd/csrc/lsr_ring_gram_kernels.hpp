// Batched ring Gram matrices in the evaluation domain (lsr_ring_gram.hip):
//   G-hat[i][l][k] = sum_{c < ncols} a-hat_i[c][k] * b-hat_l[c][k],   i < ra, l < rb, k < n.
// Every operand polynomial was transformed ONCE by launch_ntt into the context's ring workspace (canonical words, the order
// launch_ntt writes); the kernel is the pointwise product between those transforms and the inverse transforms of the outputs.  No
// LDS, no cross-lane traffic: a lane owns one evaluation position, a workgroup a run of kGramThreads positions of one family and one
// (i-block, l-block) of E x E outputs, which it keeps in registers across the columns.
//
// Grid: x = runs of positions, y = block pairs, z = families of the chunk.  Cross form: y = i-block * ceil(rb / E) + l-block.
// Symmetric form (SYM, b-hat == a-hat): only the pairs i-block <= l-block are launched, rows of the upper triangle one after the
// other, and a diagonal block stores only i <= l; output (i, l) is polynomial i r - i (i - 1) / 2 + (l - i) of the family.
// Symmetrised form (SYM2, with SYM; lsr_ntt_ring_gram_sym2_batch): ra == rb, the same block pairs and the same packed
// outputs, but output (i, l), i < l, is <a_i, b_l> + <a_l, b_i> and output (i, i) is <a_i, b_i> once.  A block pair I < L loads a_I,
// b_L, a_L and b_I per column and adds both products into the same accumulators; a diagonal block has a_L = a_I and b_I = b_L in
// registers already and skips the second product where i == l.
// Partial blocks (ra or rb no multiple of E): the counts ni, nl of live vectors are workgroup-uniform; a dead row reads the block's
// last live vector again (a uniform offset, never out of range: the same cache lines) and is not stored.  (Guarding the loads and
// products of dead rows by uniform branches instead was measured: DESIGN.md §5j.)
// Addressing: 64-bit.  The workgroup-uniform part of every address (family, vector, column) is a 64-bit scalar offset, the lane adds
// its position; a family's operands may exceed 2^31 bytes.
// Accumulator contract: ntt_tile_ring_dot's (lsr_ntt_kernels.hpp).  F64 — both operands are canonical, a product is |r| <= 0.875 q,
// the accumulator starts at 0 or at a carried-in canonical word (< q) and is re-centred every kRingDotF64Period columns (SYM2, two
// products per column: every kRingDotF64Period / 2 columns) and after the last one: |acc| <= q + 0.875 * 32 q < 2^50, exact; after
// the last re-centring |acc| <= q/2 + 1, store_reduced's domain.  U64 — canonical products and canonical sums.  Goldilocks —
// gold_add.  g always receives canonical words: the next column group loads them and adds (kRingDotFirst clear), launch_ntt's
// inverse takes them after the last group.
#pragma once
#include <type_traits>

#include "lsr_ntt_kernels.hpp"

// experiment builds only (csrc/Makefile VARIANT=..., tools/ring_gram_bench.py LIBVARIANT): the block edge of the FP64 flavour
#ifndef LSR_RING_GRAM_EDGE_F64
#define LSR_RING_GRAM_EDGE_F64 4
#endif

namespace lsr {

constexpr uint32_t kGramThreads = 256;

// Edge E of the register block per arithmetic flavour (the resource table and the measurements: DESIGN.md §5j)
template <class A> constexpr int kGramEdge = 4;
template <> inline constexpr int kGramEdge<ArithF64> = LSR_RING_GRAM_EDGE_F64;

struct GramShape {
    uint32_t logn, ra, rb, ncols, flags;   // flags: kRingDotFirst — start at zero (else: at the canonical words an earlier group left in g)
    size_t a_vec, a_fam, b_vec, b_fam;     // words between consecutive vectors / consecutive families of a-hat and b-hat
    size_t g_fam;                          // words of one family's outputs
};

// The work of one workgroup: block pair `pair` (the grid's y of the layout above) of family `fam`, both workgroup-uniform.  The kernel
// of a context passes its block indices; the kernel of a ring handle under an arbitrary modulus (lsr_ring_mod_gram_kernels.hpp) takes
// the prime out of y first.
template <class A, int E, bool SYM, bool SYM2>
__device__ __forceinline__ void ring_gram_block(uint64_t* __restrict__ g, const uint64_t* __restrict__ ahat, const uint64_t* __restrict__ bhat,
                                                const GramShape& s, const ModParams& p, uint32_t pair, uint32_t fam) {
    using elem = typename A::elem;
    const size_t n = (size_t)1 << s.logn;
    const size_t pos = (size_t)blockIdx.x * kGramThreads + threadIdx.x;
    // the block pair of this workgroup (uniform)
    const uint32_t nbl = (s.rb + E - 1) / E;
    uint32_t ib, lb;
    if constexpr (SYM) {
        uint32_t rest = pair;
        for (ib = 0; rest >= nbl - ib; ++ib) rest -= nbl - ib;
        lb = ib + rest;
    } else {
        ib = pair / nbl;
        lb = pair % nbl;
    }
    const uint32_t i0 = ib * E, l0 = lb * E;
    const uint32_t ni = min((uint32_t)E, s.ra - i0), nl = min((uint32_t)E, s.rb - l0);
    if (pos >= n) return;
    const uint64_t* const ap = ahat + fam * s.a_fam + i0 * s.a_vec;
    const uint64_t* const bp = bhat + fam * s.b_fam + l0 * s.b_vec;
    uint64_t* const gp = g + fam * s.g_fam;
    // SYM2: the transposed operands a_L and b_I of the second product (a diagonal block has them in x and y)
    static_assert(SYM || !SYM2, "the symmetrised form is a mode of the packed form");
    const bool diag = SYM2 && ib == lb;
    const uint64_t* const ap2 = ahat + fam * s.a_fam + l0 * s.a_vec;
    const uint64_t* const bp2 = bhat + fam * s.b_fam + i0 * s.b_vec;
    constexpr uint32_t kPeriod = SYM2 ? kRingDotF64Period / 2 : kRingDotF64Period;
    // (ii, ll) of the block is an output of this workgroup; its polynomial within the family
    auto live = [&](int ii, int ll) { return (uint32_t)ii < ni && (uint32_t)ll < nl && (!SYM || i0 + ii <= l0 + ll); };
    auto slot = [&](int ii, int ll) -> size_t {
        const size_t i = i0 + ii, l = l0 + ll;
        return SYM ? i * s.ra - i * (i - 1) / 2 + (l - i) : i * s.rb + l;
    };

    elem acc[E][E];
#pragma unroll
    for (int ii = 0; ii < E; ++ii)
#pragma unroll
        for (int ll = 0; ll < E; ++ll) {
            acc[ii][ll] = elem_from_bits<A>(0);
            if (!(s.flags & kRingDotFirst) && live(ii, ll)) acc[ii][ll] = A::load(gp[slot(ii, ll) * n + pos], p);
        }

    for (uint32_t c = 0; c < s.ncols; ++c) {
        const size_t col = (size_t)c << s.logn;
        elem x[E], y[E];
#pragma unroll
        for (int ii = 0; ii < E; ++ii) x[ii] = A::load(ap[min((uint32_t)ii, ni - 1u) * s.a_vec + col + pos], p);
#pragma unroll
        for (int ll = 0; ll < E; ++ll) y[ll] = A::load(bp[min((uint32_t)ll, nl - 1u) * s.b_vec + col + pos], p);
#pragma unroll
        for (int ii = 0; ii < E; ++ii)
#pragma unroll
            for (int ll = 0; ll < E; ++ll) acc[ii][ll] = ring_accumulate<A>(acc[ii][ll], ring_product<A>(x[ii], y[ll], p), p);
        if constexpr (SYM2) {
            elem xt[E], yt[E];
            if (diag) {
#pragma unroll
                for (int k = 0; k < E; ++k) xt[k] = x[k], yt[k] = y[k];
            } else {
#pragma unroll
                for (int ll = 0; ll < E; ++ll) xt[ll] = A::load(ap2[min((uint32_t)ll, nl - 1u) * s.a_vec + col + pos], p);
#pragma unroll
                for (int ii = 0; ii < E; ++ii) yt[ii] = A::load(bp2[min((uint32_t)ii, ni - 1u) * s.b_vec + col + pos], p);
            }
#pragma unroll
            for (int ii = 0; ii < E; ++ii)
#pragma unroll
                for (int ll = 0; ll < E; ++ll)
                    if (!(diag && ii == ll)) acc[ii][ll] = ring_accumulate<A>(acc[ii][ll], ring_product<A>(xt[ll], yt[ii], p), p);
        }
        if constexpr (std::is_same_v<A, ArithF64>) {
            if ((c & (kPeriod - 1u)) == kPeriod - 1u || c + 1 == s.ncols) {
#pragma unroll
                for (int ii = 0; ii < E; ++ii)
#pragma unroll
                    for (int ll = 0; ll < E; ++ll) acc[ii][ll] = recentre_f64(acc[ii][ll], p.qd, p.inv_qd);
            }
        }
    }

#pragma unroll
    for (int ii = 0; ii < E; ++ii)
#pragma unroll
        for (int ll = 0; ll < E; ++ll)
            if (live(ii, ll)) gp[slot(ii, ll) * n + pos] = A::store_reduced(acc[ii][ll], p);
}

template <class A, int E, bool SYM, bool SYM2 = false>
__global__ void __launch_bounds__(kGramThreads) ring_gram_kernel(uint64_t* __restrict__ g, const uint64_t* __restrict__ ahat,
                                                                   const uint64_t* __restrict__ bhat, GramShape s, ModParams p) {
    ring_gram_block<A, E, SYM, SYM2>(g, ahat, bhat, s, p, blockIdx.y, blockIdx.z);
}

}  // namespace lsr
