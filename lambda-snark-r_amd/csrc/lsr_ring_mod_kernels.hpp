// The two streaming kernels of a ring handle under an arbitrary modulus q (lsr_ring_mod.hip, batch.h "ring products under any
// modulus"): `lift` takes words mod q to the canonical residues mod one of the handle's two NTT primes of their
// centred representatives, `reduce` takes a pair of residues back to the word mod q of the integer they determine in
// [-(P - 1) / 2, (P - 1) / 2], P = p1 p2.  Both are one pass without a workspace, at any count (they run no transform): 16 bytes per
// lane and access where every buffer is 16-byte aligned, 8 bytes otherwise.  (The fused inner product lifts as it loads:
// ntt_tile_ring_dot_lift, lsr_ring_galois_kernels.hpp.)
// Behind them the two kernels that the bounded calls of a handle share (Gram, fold, quadratic forms, the bounded matrix product;
// launched by lsr_ring_mod_call.hpp): ring_mod_gram_lift_kernel, the lift for both primes with the caller's bound
// verified into a flag word per family, and ring_mod_gram_reduce_kernel, the reduce gated by those flags.
#pragma once

#include "lsr_ring_galois_kernels.hpp"

namespace lsr {

constexpr uint32_t kRingModThreads = 256;

// constants of one handle (host-built, passed by value)
struct RingModConsts {
    uint64_t p[2];               // p1, p2 in (2^43, 2^44)
    uint64_t p1inv;              // p1^-1 mod p2
    uint64_t half_lo, half_hi;   // (P - 1) / 2 < 2^87
    uint64_t p1_mod_q, big_mod_q;   // p1 mod q, P mod q
};

// x mod q for any 64-bit x, from the high word of floor(2^128 / q), which is floor(2^64 / q) =: m.  x m / 2^64 > x / q - x / 2^64 >
// x / q - 1, so the estimate umulhi(x, m) is floor(x / q) or one less and the remainder lies in [0, 2 q); q < 2^45 here.
__device__ __forceinline__ uint64_t mod64_barrett(uint64_t x, const ModParams& p) {
    const uint64_t r = x - __umul64hi(x, p.barrett_hi) * p.q;
    return r >= p.q ? r - p.q : r;
}

// Residues r0 < p1, r1 < p2 of the integer X in [-(P - 1) / 2, (P - 1) / 2] -> X mod q in [0, q).  Garner, as rns_decode_slot
// (lsr_commit_rns.hpp):
//   r0' = r0 mod p2                      one conditional subtraction (r0 < 2^44 < 2 p2)
//   y   = (r1 - r0') p1^-1 mod p2        Barrett product mod p2, y < p2
//   X'  = r0 + p1 y                      the representative in [0, P)                 (128-bit, only compared)
//   X   = X' - [X' > (P - 1) / 2] P
// and from there mod q, where no 128-bit division is needed: X = r0 + p1 y - [.] P, every term reduced mod q on its own (p2 and pq
// are ModParams of p2 and of q; floor(2^128 / q) needs no primality).  The sum of two residues stays below 2 q < 2^46.
__device__ __forceinline__ uint64_t ring_mod_reduce_word(uint64_t r0, uint64_t r1, const RingModConsts& rc, const ModParams& p2, const ModParams& pq) {
    const uint64_t r0r = r0 >= rc.p[1] ? r0 - rc.p[1] : r0;
    const uint64_t diff = r1 >= r0r ? r1 - r0r : r1 + rc.p[1] - r0r;
    const uint64_t y = mulmod_barrett128(diff, rc.p1inv, p2);
    const unsigned __int128 x = (unsigned __int128)rc.p[0] * y + r0;
    const unsigned __int128 half = ((unsigned __int128)rc.half_hi << 64) | rc.half_lo;
    uint64_t s = mod64_barrett(r0, pq) + mulmod_barrett128(y, rc.p1_mod_q, pq);
    s = s >= pq.q ? s - pq.q : s;
    if (x > half) s = s >= rc.big_mod_q ? s - rc.big_mod_q : s + pq.q - rc.big_mod_q;
    return s;
}
__device__ __forceinline__ uint64_t ring_mod_add(uint64_t a, uint64_t b, uint64_t q) {   // a, b < q < 2^45
    const uint64_t s = a + b;
    return s >= q ? s - q : s;
}

// out[e] = lift(x[e]) for e < count.  out may be x itself (no __restrict__: a lane reads its words before it writes them, and no
// lane touches another lane's).  VEC: both buffers 16-byte aligned — a lane takes pairs of words, lane 0 of workgroup 0 the odd
// word left over.
template <bool VEC>
__global__ void __launch_bounds__(kRingModThreads) ring_mod_lift_kernel(uint64_t* out, const uint64_t* x, size_t count, LiftSource lift) {
    const size_t stride = (size_t)gridDim.x * kRingModThreads, first = (size_t)blockIdx.x * kRingModThreads + threadIdx.x;
    if constexpr (VEC) {
        const size_t pairs = count >> 1;
        for (size_t e = first; e < pairs; e += stride) {
            ulonglong2 v = reinterpret_cast<const ulonglong2*>(x)[e];
            v.x = lift.word(v.x);
            v.y = lift.word(v.y);
            reinterpret_cast<ulonglong2*>(out)[e] = v;
        }
        if ((count & 1) && first == 0) out[count - 1] = lift.word(x[count - 1]);
    } else {
        for (size_t e = first; e < count; e += stride) out[e] = lift.word(x[e]);
    }
}

// out[e] = reduce(r0[e], r1[e]) for e < count, ACC: added mod q to the word out[e] holds.  VEC as above (all three buffers).  out
// may be r0 or r1 itself (no __restrict__, as above).
template <bool VEC, bool ACC>
__global__ void __launch_bounds__(kRingModThreads) ring_mod_reduce_kernel(uint64_t* out, const uint64_t* r0, const uint64_t* r1, size_t count,
                                                                           RingModConsts rc, ModParams p2, ModParams pq) {
    const size_t stride = (size_t)gridDim.x * kRingModThreads, first = (size_t)blockIdx.x * kRingModThreads + threadIdx.x;
    auto word = [&](size_t e) {
        const uint64_t v = ring_mod_reduce_word(r0[e], r1[e], rc, p2, pq);
        out[e] = ACC ? ring_mod_add(out[e], v, pq.q) : v;
    };
    if constexpr (VEC) {
        const size_t pairs = count >> 1;
        for (size_t e = first; e < pairs; e += stride) {
            const ulonglong2 a = reinterpret_cast<const ulonglong2*>(r0)[e], b = reinterpret_cast<const ulonglong2*>(r1)[e];
            ulonglong2 v;
            v.x = ring_mod_reduce_word(a.x, b.x, rc, p2, pq);
            v.y = ring_mod_reduce_word(a.y, b.y, rc, p2, pq);
            if constexpr (ACC) {
                const ulonglong2 old = reinterpret_cast<const ulonglong2*>(out)[e];
                v.x = ring_mod_add(old.x, v.x, pq.q);
                v.y = ring_mod_add(old.y, v.y, pq.q);
            }
            reinterpret_cast<ulonglong2*>(out)[e] = v;
        }
        if ((count & 1) && first == 0) word(count - 1);
    } else {
        for (size_t e = first; e < count; e += stride) word(e);
    }
}

// The checked lift: one read of every operand word, its centred representative as the canonical residue mod p1 and mod p2 into the
// two halves of a workspace, and "over the bound" / ">= q" folded into one flag word per family.  Grid: x = runs of a vector's words
// (grid-stride), y = vectors, z = families — every stride is a scalar offset, no lane divides.  16 bytes per lane and access where the
// source is 16-byte aligned (the workspace always is; every run and stride is a multiple of n >= 2 words).  CHECK: fold the flags (a
// wave ORs its lanes' bits first, then at most one atomic OR per wave); STORE: write the residues.  A family taken in several groups
// is checked whole by a pass without STORE before its first group, so that its flags are complete before any reduce reads them.
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

// The gated reduce: ring_mod_reduce_kernel with the family as grid y — the word mod q of the integer a pair of residues determines
// (ACC: added to what g holds), or 0 — whatever ACC says — where the family's flags are set; lane 0 of a family's first workgroup
// writes status[family].  g: [families][words] (words even), r0 / r1: the families `r_fam` words apart
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
