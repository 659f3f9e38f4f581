// Ring quadratic forms of a packed symmetric matrix in the evaluation domain (lsr_ring_quadform.hip):
//   Q-hat[k] = sum_i c-hat_i[k] * ( g-hat_ii[k] * c-hat_i[k] + offdiag * sum_{l > i} g-hat_il[k] * c-hat_l[k] ),   k < n,
// evaluated row by row of the triangle: pairs + 2 r products per position instead of the 2 pairs of a product per pair.  g-hat and
// c-hat were transformed by launch_ntt into the context's ring workspace (canonical words, the order launch_ntt writes).  No LDS, no
// cross-lane traffic: a lane owns one evaluation position.
//
// Grid: x = runs of kQuadThreads positions, y = slices of the triangle, z = families of the chunk.  The launch covers the packed pairs
// [p_begin, p_end) of the triangle (the whole triangle, or one group of a family that does not fit the workspace); slice y takes the
// pairs p_begin + [y count / slices, (y + 1) count / slices): slices are balanced by PAIRS and may start and end inside a row.  A
// piece (l0 <= l < l1) of row i contributes c-hat_i * ([l0 == i] g-hat_ii c-hat_i + offdiag * sum_{max(l0, i + 1) <= l < l1} g-hat_il
// c-hat_l); the sum is linear in the pieces, every word written is the canonical residue, and residues are unique: the result does
// not depend on the slicing.
// One slice: the lane adds the carried-in sum (kRingDotFirst clear: the canonical words an earlier group left in out) and stores the
// canonical sum to out.  More slices: each stores its canonical partial to part[family][slice][n] in the workspace and
// ring_quadform_reduce_kernel adds carried-in sum and slices in slice order.  No atomics.
// Addressing: plain 64-bit loads; the workgroup-uniform part of every address (family, pair, vector) is a 64-bit scalar offset.  g-hat
// is read once, coalesced; c-hat_l is re-read per row from cache (r n words per family).
// Exactness per flavour: DESIGN.md §5m.  F64 — every mulmod_f64 has one canonical operand (c-hat_l, c-hat_i, offdiag: loaded words
// below q) and the other |x| < 2^50; a product is |r| <= 0.875 q; the inner sum is re-centred every kRingDotF64Period products and
// before the outer multiplies (|inner| <= q/2 + 1 + 28 q < 2^50), the diagonal product plus the scaled inner sum is |u| <= 1.75 q, the
// outer sum starts at 0 or a canonical word and is re-centred every kRingDotF64Period rows and after the last one, store_reduced's
// domain.  U64 — canonical products (Barrett) and canonical sums.  Goldilocks — gold_mul / gold_add.
#pragma once
#include <type_traits>

#include "lsr_ntt_kernels.hpp"

// experiment builds only (csrc/Makefile VARIANT=..., tools/ring_quadform_bench.py LIBVARIANT): the unrolling of the inner sum of a row
#ifndef LSR_RING_QUADFORM_UNROLL
#define LSR_RING_QUADFORM_UNROLL 4
#endif

namespace lsr {

constexpr uint32_t kQuadThreads = 256;

struct QuadShape {
    uint32_t logn, r, flags;      // flags: kRingDotFirst — start at zero (else: at the canonical words an earlier group left in out)
    uint32_t p_begin, p_end;      // the packed pairs this launch covers; g-hat holds them from p_begin on
    uint32_t slices;              // == gridDim.y
    size_t c_fam, g_fam;          // words between consecutive families of c-hat (0: one shared set) and of g-hat
    uint64_t offdiag;             // canonical word
};

// x * y for a canonical y (and |x| < 2^50 in the F64 flavour); F64: |r| <= 0.875 q, else canonical
template <class A>
__device__ __forceinline__ typename A::elem quad_product(typename A::elem x, typename A::elem y, const ModParams& p) {
    if constexpr (std::is_same_v<A, ArithF64>) return mulmod_f64(x, y, p.qd, p.inv_qd);
    else return ring_product<A>(x, y, p);
}

template <class A>
__global__ void __launch_bounds__(kQuadThreads) ring_quadform_kernel(uint64_t* __restrict__ out, uint64_t* __restrict__ part,
                                                                      const uint64_t* __restrict__ ghat, const uint64_t* __restrict__ chat,
                                                                      QuadShape s, ModParams p) {
    using elem = typename A::elem;
    constexpr bool kF64 = std::is_same_v<A, ArithF64>;
    const size_t n = (size_t)1 << s.logn;
    const size_t pos = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= n) return;
    // the pairs of this slice (uniform), and the row and column of the first one
    const uint32_t count = s.p_end - s.p_begin;
    const uint32_t p0 = s.p_begin + (uint32_t)((uint64_t)blockIdx.y * count / s.slices);
    const uint32_t p1 = s.p_begin + (uint32_t)((uint64_t)(blockIdx.y + 1) * count / s.slices);
    uint32_t i = 0, rest = p0;
    for (; i < s.r && rest >= s.r - i; ++i) rest -= s.r - i;     // (slices <= count: p0 is a pair of the triangle)
    uint32_t l = i + rest;

    const uint64_t* const cp = chat + blockIdx.z * s.c_fam + pos;
    const uint64_t* gp = ghat + blockIdx.z * s.g_fam + ((size_t)(p0 - s.p_begin) << s.logn) + pos;
    const elem off = A::load(s.offdiag, p);

    elem acc = elem_from_bits<A>(0);
    if (s.slices == 1 && !(s.flags & kRingDotFirst)) acc = A::load(out[blockIdx.z * n + pos], p);
    uint32_t rows = 0;
    for (uint32_t pp = p0; pp < p1; ++i, l = i) {
        const uint32_t row_end = min(p1, pp + (s.r - l));
        const elem ci = A::load(cp[(size_t)i << s.logn], p);
        elem diag = elem_from_bits<A>(0), inner = elem_from_bits<A>(0);
        if (l == i) {
            diag = quad_product<A>(A::load(*gp, p), ci, p);
            gp += n, ++pp, ++l;
        }
#pragma unroll LSR_RING_QUADFORM_UNROLL
        for (uint32_t t = 0; pp < row_end; ++pp, ++l, ++t, gp += n) {
            inner = ring_accumulate<A>(inner, quad_product<A>(A::load(*gp, p), A::load(cp[(size_t)l << s.logn], p), p), p);
            if constexpr (kF64) {
                if ((t & (kRingDotF64Period - 1u)) == kRingDotF64Period - 1u) inner = recentre_f64(inner, p.qd, p.inv_qd);
            }
        }
        if constexpr (kF64) inner = recentre_f64(inner, p.qd, p.inv_qd);
        const elem u = ring_accumulate<A>(diag, quad_product<A>(inner, off, p), p);
        acc = ring_accumulate<A>(acc, quad_product<A>(u, ci, p), p);
        if constexpr (kF64) {
            if ((++rows & (kRingDotF64Period - 1u)) == 0) acc = recentre_f64(acc, p.qd, p.inv_qd);
        }
    }
    if constexpr (kF64) acc = recentre_f64(acc, p.qd, p.inv_qd);
    uint64_t* const to = s.slices == 1 ? out + blockIdx.z * n : part + ((size_t)blockIdx.z * s.slices + blockIdx.y) * n;
    to[pos] = A::store_reduced(acc, p);
}

// out[family] = (kRingDotFirst clear: out[family]) + part[family][0] + ... + part[family][slices - 1], canonical words in and out,
// in this order.  GOLD: gold_add; else one conditional subtraction per sum (q < 2^61).
template <bool GOLD>
__global__ void __launch_bounds__(kQuadThreads) ring_quadform_reduce_kernel(uint64_t* __restrict__ out, const uint64_t* __restrict__ part,
                                                                             uint32_t logn, uint32_t slices, uint32_t flags, uint64_t q) {
    const size_t n = (size_t)1 << logn;
    const size_t pos = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= n) return;
    uint64_t* const to = out + blockIdx.y * n + pos;
    const uint64_t* from = part + (size_t)blockIdx.y * slices * n + pos;
    uint64_t acc = (flags & kRingDotFirst) ? 0 : *to;
    // (unrolled: the loads of eight slices are in flight together; one at a time the loop waits out a memory latency per slice)
#pragma unroll 8
    for (uint32_t t = 0; t < slices; ++t, from += n) {
        if constexpr (GOLD) {
            acc = gold_add(acc, *from);
        } else {
            acc += *from;
            acc = acc >= q ? acc - q : acc;
        }
    }
    *to = acc;
}

}  // namespace lsr
