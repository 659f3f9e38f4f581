// Scalar-weighted aggregation of ring vectors with an addend (batch.h "scalar-weighted aggregation of ring vectors"):
//   out[j][k][pos] = (addend ? addend[j][k][pos] : 0) + sum_{i < terms} weights[j / components][k][i] v[j term_stride + i][pos]  mod q.
// A scalar acts coefficient-wise: no transform, no twiddle table, a tall-skinny modular matrix product streamed over v.
//   A workgroup of 256 lanes owns a tile of positions of one vector j for one block of LIVE <= kScalarSetBlock sets; a lane owns P
//   consecutive positions: P = 2 with 16-byte loads and stores (kScalarTile = 512 positions) when v, out and addend are 16-byte
//   aligned, else P = 1 with 8-byte ones.  It walks the terms with one coalesced load of v per term; a loaded word (converted once,
//   whatever the number of sets) feeds one accumulator per set of the block.  LIVE is a template argument: a call of 3 sets runs the
//   instantiation of 3, with the registers and the LDS of 3.  The weights of the (group, set block) are the same in every lane:
//   kScalarStage terms at a time are brought into the flavour's multiplier form by one lane each (a double; a Shoup operand; the
//   Montgomery form) and staged in LDS as [term][set], where every lane of a wavefront reads the same address — a broadcast.
//   Every workgroup tests all sets * terms weight words of its group against q on the way in (they are few beside terms * 256 words
//   of v): one kernel writes every output word and the status, no init pass, no atomics.
// Exactness per flavour (§5l): F64 — |acc| <= q + 32 * 0.875 q = 29 q < 2^50 between re-centrings, 32 q at the canonical store;
// U64 — lazy Shoup products in [0, 2q) added to an accumulator kept in [0, 2q): below 4q < 2^63; Goldilocks — canonical throughout.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "lsr_arith.hpp"
#include "lsr_ntt_kernels.hpp"      // kRingDotF64Period

namespace lsr {

#ifndef LSR_SCALAR_SET_BLOCK
#define LSR_SCALAR_SET_BLOCK 16                   // the most sets accumulated per pass over v (1, 2, 4, 8 or 16; timed in §5l)
#endif
#ifndef LSR_SCALAR_POSITIONS
#define LSR_SCALAR_POSITIONS 2                    // the most positions per lane (1 or 2; timed in §5l)
#endif
#ifndef LSR_SCALAR_UNROLL
#define LSR_SCALAR_UNROLL 4                       // terms whose loads are in flight together
#endif
constexpr int kScalarSetBlock = LSR_SCALAR_SET_BLOCK;
constexpr int kScalarMaxSets = 16;                // LSR_RING_SCALAR_COMBINE_MAX_SETS
constexpr int kScalarThreads = 256;
constexpr int kScalarPositions = LSR_SCALAR_POSITIONS;
constexpr uint32_t kScalarTile = kScalarThreads * kScalarPositions;      // positions per workgroup at the most positions per lane
constexpr uint32_t kScalarStage = 128;            // terms whose weights are staged at a time
static_assert(kScalarSetBlock == 1 || kScalarSetBlock == 2 || kScalarSetBlock == 4 || kScalarSetBlock == 8 || kScalarSetBlock == 16,
              "the set block is 1, 2, 4, 8 or 16");
static_assert(kScalarPositions == 1 || kScalarPositions == 2, "a lane owns one position or two");
static_assert(kScalarStage % kRingDotF64Period == 0, "a stage is whole re-centring periods: the period counts from the stage's first term");

// The arithmetic of one flavour: weight — the staged multiplier; word — a word of v as the steps take it; acc — a running sum.
template <class A> struct ScalarOps;

template <> struct ScalarOps<ArithF64> {
    using weight = double;
    using word = double;
    using acc = double;
    static constexpr bool kSettles = true;
    static __device__ __forceinline__ weight prepare(uint64_t w, const ModParams&) { return f64_from_u52(w); }
    static __device__ __forceinline__ word operand(uint64_t x, const ModParams&) { return f64_from_u52(x); }
    static __device__ __forceinline__ acc start(uint64_t addend, const ModParams&) { return f64_from_u52(addend); }      // [0, q)
    // a product of magnitude <= 0.875 q (lsr_arith.hpp mulmod_f64) onto an exact integer
    static __device__ __forceinline__ void step(acc& a, word x, weight w, const ModParams& p) { a += mulmod_f64(x, w, p.qd, p.inv_qd); }
    // every kRingDotF64Period products: back to |a| <= q / 2 + 1
    static __device__ __forceinline__ void settle(acc& a, const ModParams& p) { a = recentre_f64(a, p.qd, p.inv_qd); }
    // at most 32 products since the addend (< q) or a re-centring: |a| <= 29 q, inside canonical_f64's |v| <= 32 q
    static __device__ __forceinline__ uint64_t finish(acc a, const ModParams& p) { return u52_from_f64(canonical_f64(a, p.qd, p.inv_qd)); }
};

template <> struct ScalarOps<ArithU64> {
    using weight = ShoupOperand;
    using word = uint64_t;
    using acc = uint64_t;
    static constexpr bool kSettles = false;
    // floor(w 2^64 / q) for w < q from floor(2^128 / q) = (bhi, blo): e = w bhi + floor(w blo / 2^64) is that quotient or one less
    // (floor(2^128 / q) falls short of 2^128 / q by less than 1, w / 2^64 of that is less than 1), and w 2^64 - e q, below 2 q, tells
    static __device__ __forceinline__ weight prepare(uint64_t w, const ModParams& p) {
        uint64_t e = w * p.barrett_hi + __umul64hi(w, p.barrett_lo);
        if (0ull - e * p.q >= p.q) ++e;
        return {w, e};
    }
    static __device__ __forceinline__ word operand(uint64_t x, const ModParams&) { return x; }
    static __device__ __forceinline__ acc start(uint64_t addend, const ModParams&) { return addend; }                   // [0, q)
    // a in [0, 2q) and a lazy product in [0, 2q) (any 64-bit x): the sum is below 4q < 2^63; one conditional subtraction
    static __device__ __forceinline__ void step(acc& a, word x, weight w, const ModParams& p) {
        const uint64_t s = a + mul_shoup_lazy(x, w, p.q);
        a = s >= p.two_q ? s - p.two_q : s;
    }
    static __device__ __forceinline__ void settle(acc&, const ModParams&) {}
    static __device__ __forceinline__ uint64_t finish(acc a, const ModParams& p) { return a >= p.q ? a - p.q : a; }
};

template <> struct ScalarOps<ArithGold> {
    using weight = uint64_t;      // Montgomery form
    using word = uint64_t;
    using acc = uint64_t;
    static constexpr bool kSettles = false;
    static __device__ __forceinline__ weight prepare(uint64_t w, const ModParams&) { return gold_mul(w, kGoldEpsilon); }   // w 2^64 mod p
    static __device__ __forceinline__ word operand(uint64_t x, const ModParams&) { return x; }
    static __device__ __forceinline__ acc start(uint64_t addend, const ModParams&) { return addend >= kGoldilocks ? addend - kGoldilocks : addend; }
    // gold_mul_mont: canonical for any 64-bit x; gold_add of two canonical words
    static __device__ __forceinline__ void step(acc& a, word x, weight w, const ModParams&) { a = gold_add(a, gold_mul_mont(x, w)); }
    static __device__ __forceinline__ void settle(acc&, const ModParams&) {}
    static __device__ __forceinline__ uint64_t finish(acc a, const ModParams&) { return a; }
};

struct ScalarCombineJob {
    uint64_t* out;            // [count][sets][len], vector `first` of the call at out
    int32_t* status;          // [count]
    const uint64_t* v;        // [vectors][len], term 0 of vector `first` at v
    const uint64_t* weights;  // [groups][sets][terms], the group of vector j at weights + (j / components - group_base) sets terms
    const uint64_t* addend;   // NULL, or laid out as out (and then possibly out itself)
    uint64_t components;
    uint64_t group_base;      // the first weight group present at `weights` (host staging uploads the groups of one chunk)
    uint64_t first;           // vectors [first, first + gridDim.x / (tiles set_blocks)) of the call
    uint64_t len;             // width n, at most 2^32
    uint64_t term_stride;     // vectors between the first terms of consecutive outputs
    uint32_t terms;           // at most 65536
    uint32_t sets;
    uint32_t tiles;           // ceil(len / (256 P)): at most 2^24
    uint32_t set_first;       // this launch covers the sets [set_first, set_first + LIVE set_blocks)
    uint32_t set_blocks;
};

// P consecutive words, as one 8-byte or one 16-byte access (P = 2: the address is 16-byte aligned)
template <int P>
__device__ __forceinline__ void scalar_load(const uint64_t* from, uint64_t (&x)[P]) {
    if constexpr (P == 2) {
        const ulonglong2 w = *reinterpret_cast<const ulonglong2*>(from);
        x[0] = w.x;
        x[1] = w.y;
    } else {
        x[0] = *from;
    }
}
template <int P>
__device__ __forceinline__ void scalar_store(uint64_t* to, const uint64_t (&x)[P]) {
    if constexpr (P == 2) *reinterpret_cast<ulonglong2*>(to) = make_ulonglong2(x[0], x[1]);
    else *to = x[0];
}

// workgroup (vector, tile, set block), the set blocks of one tile next to each other: positions [256 P tile, 256 P (tile + 1)) of one
// vector for the sets [set_first + LIVE block, + LIVE).  The launches of a call write every output word and the status themselves.
template <class A, int LIVE, int P>
__global__ void __launch_bounds__(kScalarThreads) ring_scalar_combine_kernel(ScalarCombineJob job, ModParams p) {
    using Ops = ScalarOps<A>;
    __shared__ typename Ops::weight wt[kScalarStage * LIVE];                     // [term][set]
    const uint32_t t = threadIdx.x;
    const uint32_t per_vector = job.tiles * job.set_blocks;                      // at most 2^28
    const uint32_t local = blockIdx.x / per_vector, rest = blockIdx.x - local * per_vector;
    const uint32_t tile = rest / job.set_blocks, k0 = job.set_first + (rest - tile * job.set_blocks) * LIVE;
    const uint64_t len = job.len;
    const uint64_t group = (job.first + local) / job.components - job.group_base;
    const uint64_t* __restrict__ wg = job.weights + group * job.sets * job.terms;
    bool not_below_q = false;
    for (uint32_t e = t; e < job.sets * job.terms; e += kScalarThreads) not_below_q |= wg[e] >= p.q;      // at most 2^20 words
    not_below_q = __syncthreads_or(not_below_q);
    if (rest == 0 && job.set_first == 0 && t == 0) job.status[local] = not_below_q ? -1 : 1;

    // a lane behind the vector's end works on the last positions and stores nothing (P = 2: len is even, a pair is live or not)
    const uint64_t pos = ((uint64_t)tile * kScalarThreads + t) * P;
    const bool live = pos < len;
    const uint64_t o = ((uint64_t)local * job.sets + k0) * len + (live ? pos : len - P);      // set k0 of this lane in out and addend
    if (not_below_q) {                                // the same in every lane of the workgroup
        const uint64_t zero[P] = {};
        if (live)
            for (int k = 0; k < LIVE; ++k) scalar_store<P>(job.out + o + (uint64_t)k * len, zero);
        return;
    }
    typename Ops::acc sum[LIVE][P];
#pragma unroll
    for (int k = 0; k < LIVE; ++k) {
        uint64_t a[P] = {};
        if (job.addend) scalar_load<P>(job.addend + o + (uint64_t)k * len, a);
#pragma unroll
        for (int e = 0; e < P; ++e) sum[k][e] = Ops::start(a[e], p);
    }
    const uint64_t* __restrict__ src = job.v + (uint64_t)local * job.term_stride * len + (live ? pos : len - P);
    wg += (uint64_t)k0 * job.terms;
    for (uint32_t i0 = 0; i0 < job.terms; i0 += kScalarStage) {
        const uint32_t now = min(kScalarStage, job.terms - i0);
        if (i0) __syncthreads();                      // the previous stage has been read
        for (uint32_t e = t; e < kScalarStage * LIVE; e += kScalarThreads) {      // consecutive lanes, consecutive terms of one set
            const uint32_t k = e / kScalarStage, i = e % kScalarStage;
            if (i < now) wt[i * LIVE + k] = Ops::prepare(wg[(uint64_t)k * job.terms + i0 + i], p);
        }
        __syncthreads();
        const uint64_t* __restrict__ at = src + (uint64_t)i0 * len;
#pragma unroll LSR_SCALAR_UNROLL
        for (uint32_t i = 0; i < now; ++i) {
            uint64_t raw[P];
            scalar_load<P>(at + (uint64_t)i * len, raw);
            typename Ops::word x[P];
#pragma unroll
            for (int e = 0; e < P; ++e) x[e] = Ops::operand(raw[e], p);
#pragma unroll
            for (int k = 0; k < LIVE; ++k) {
                const typename Ops::weight w = wt[i * LIVE + k];      // the same address in every lane: a broadcast
#pragma unroll
                for (int e = 0; e < P; ++e) Ops::step(sum[k][e], x[e], w, p);
            }
            if constexpr (Ops::kSettles) {
                if ((i & (kRingDotF64Period - 1u)) == kRingDotF64Period - 1u) {
#pragma unroll
                    for (int k = 0; k < LIVE; ++k)
#pragma unroll
                        for (int e = 0; e < P; ++e) Ops::settle(sum[k][e], p);
                }
            }
        }
    }
    if (live) {
#pragma unroll
        for (int k = 0; k < LIVE; ++k) {
            uint64_t r[P];
#pragma unroll
            for (int e = 0; e < P; ++e) r[e] = Ops::finish(sum[k][e], p);
            scalar_store<P>(job.out + o + (uint64_t)k * len, r);
        }
    }
}

}  // namespace lsr
