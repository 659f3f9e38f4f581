// Galois automorphisms sigma_g: X -> X^g of Z_q[X]/(X^n + 1) (negacyclic contexts, N = 2 n) and Z_q[X]/(X^n - 1) (cyclic contexts,
// N = n), for odd g in [1, N) (lsr_ring_galois.hip, batch.h "Galois automorphisms").  In gather form, with
// h = g^-1 mod N and s = (j h) mod N:   out[j] = x[s]  (s < n),   out[j] = -x[s - n]  (s >= n; negacyclic only).
// Both rings share one expression: s = (j h) & (N - 1), source word s & (n - 1), negated where s & n — bit log n of s is inside the
// mask N - 1 on a negacyclic context only.  N is a power of two dividing 2^32, so the 32-bit product j h masked with N - 1 is exact
// although j h itself passes 2^32 (n up to 2^22: j < 2^22, h < 2^23).
#pragma once

#include "lsr_ntt_kernels.hpp"

namespace lsr {

// h = g^-1 mod N and the mask N - 1, computed on the host
struct GaloisParams {
    uint32_t h;
    uint32_t mask;
};

// the canonical word of -x for a canonical x
__device__ __forceinline__ uint64_t galois_negate(uint64_t x, uint64_t q) { return x ? q - x : 0ull; }

// out[e] = sigma_g(x[e]); `total` = count n words.  One workgroup takes runs of 4096 consecutive output words (16 per lane, each
// store instruction of a wave covering 64 consecutive words), so every range a buffer resource spans is one run or one polynomial
// behind a 64-bit base, whatever count n is.
//   STAGED (n <= 4096): the run is 4096 / n whole polynomials (fewer in a ragged last run: the resource ranges clip it).  It is read
//       in 16-byte pieces in order into LDS, and the permuted read is the LDS read.  The image is NOT padded: the 32 lanes of a
//       ds_read_b64 group read words (j0 + l) h of their polynomials, and with h odd these are 32 different residues mod 32 — for
//       n < 32 the group covers 32 / n whole polynomials, each a permutation of its own n words — so every odd h is free of bank
//       conflicts; a padded image would lose that.
//   else (n > 4096): the run lies inside one polynomial and every lane gathers its 16 source words from memory (stride h words:
//       one word per cache line fetched, the lines shared with other runs of the polynomial through L2).
template <bool STAGED>
__global__ void __launch_bounds__(kThreads) ring_automorphism_kernel(uint64_t* __restrict__ out, const uint64_t* __restrict__ x, size_t total, int logn,
                                                                       GaloisParams g, uint64_t q) {
    __shared__ __align__(16) uint64_t lds[STAGED ? kTile : 1];
    const uint32_t t = threadIdx.x;
    const uint32_t n = 1u << logn, nmask = n - 1u;
    const size_t runs = (total + kTile - 1) / kTile;
    for (size_t run = blockIdx.x; run < runs; run += gridDim.x) {
        const size_t base = run * kTile;
        const size_t left = total - base;
        const uint32_t words = left >= kTile ? kTile : (uint32_t)left;
        const rsrc_t rout = make_rsrc(out + base, words * 8u);
        uint64_t v[kRegs];
        if constexpr (STAGED) {
            const rsrc_t rin = make_rsrc(x + base, words * 8u);
#pragma unroll
            for (int k = 0; k < kRegs / 2; ++k) buf_load128(rin, t * 16u, (uint32_t)k * kThreads * 16u, v[2 * k], v[2 * k + 1]);
#pragma unroll
            for (int k = 0; k < kRegs / 2; ++k) {
                lds[2u * (t + (uint32_t)k * kThreads)] = v[2 * k];
                lds[2u * (t + (uint32_t)k * kThreads) + 1u] = v[2 * k + 1];
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < kRegs; ++k) {
                const uint32_t idx = t + (uint32_t)k * kThreads;
                const uint32_t s = ((idx & nmask) * g.h) & g.mask;
                const uint64_t w = lds[(idx & ~nmask) | (s & nmask)];
                v[k] = (s & n) ? galois_negate(w, q) : w;
            }
            __syncthreads();   // the image is written again for the workgroup's next run
        } else {
            const uint32_t pos = (uint32_t)(base & nmask);   // of the run in its polynomial (n is a multiple of 4096)
            const rsrc_t rin = make_rsrc(x + (base - pos), 8u << logn);
            uint32_t s[kRegs];
#pragma unroll
            for (int k = 0; k < kRegs; ++k) {
                s[k] = ((pos + t + (uint32_t)k * kThreads) * g.h) & g.mask;
                v[k] = buf_load64(rin, (s[k] & nmask) * 8u, 0);
            }
#pragma unroll
            for (int k = 0; k < kRegs; ++k) v[k] = (s[k] & n) ? galois_negate(v[k], q) : v[k];
        }
#pragma unroll
        for (int k = 0; k < kRegs; ++k) buf_store64<kAuxStream>(rout, t * 8u, (uint32_t)k * kThreads * 8u, v[k]);
    }
}

// c_j = sum_{i < nterms} sigma_g(a_{j,i}) b_{j,i}: ntt_tile_ring_dot<A, LT, MID = false, BHAT> (lsr_ntt_kernels.hpp) with the words of
// a fetched through the permutation.  Schedule, accumulator contract, kRingDotFirst / kRingDotLast hand-over and inverse rounds are
// that kernel's; b, b-hat and c are addressed as there.  The loader handed to ring_forward_tile_from returns, for tile index
// idx = output (idx >> LT) | coefficient j (idx & (n - 1)), the canonical word of sigma_g(a)[j]: everything behind the load is the
// plain kernel's instruction sequence on the operands the plain kernel would read from a materialised sigma_g(a), so c equals
// ring_dot(automorphism(a), b) word for word, and the exactness argument of DESIGN.md §5c holds unchanged (the loaded operand is a
// canonical ring element either way).
// The permutation acts on the coefficient bits only: j h = (lane part + register part) h, the register part's product is
// workgroup-uniform, so a word costs one add and one mask over the plain kernel's addressing — but lane and register parts no longer
// split in the SOURCE offset, which is one per-lane byte offset.  The ragged-tile clips survive: the resource spans the outputs the
// tile has, and a word of an absent output gets the out-of-range lane offset (reads 0; -0 = 0).
//
// The body is shared with the lift-on-load families below through a word source `Src`:
//   Src::kPermuted   the words of a are fetched through src.g (GaloisSource, LiftGaloisSource) or at the plain kernel's addresses
//                    (LiftSource);
//   Src::kLifted     every raw operand word of a and b goes through src.word(x) before A::load (LiftSource, LiftGaloisSource).
struct GaloisSource {
    static constexpr bool kPermuted = true;
    static constexpr bool kLifted = false;
    GaloisParams g;
    __device__ __forceinline__ uint32_t lane_product(uint32_t j) const { return j * g.h; }   // the lane part of j h
};
// A word x in [0, q) of a ring element mod q as the canonical residue mod a prime p of its centred representative (lsr_ring_mod.hip,
// DESIGN.md §5p): x itself up to half = floor(q / 2), else x - q + p.  rebase = p - q mod 2^64; the sum wraps to the true value,
// which lies in (p - half, p) because half < 2^43 < p.
struct LiftSource {
    static constexpr bool kPermuted = false;
    static constexpr bool kLifted = true;
    uint64_t half, rebase;
    __device__ __forceinline__ uint32_t lane_product(uint32_t) const { return 0u; }
    __device__ __forceinline__ uint64_t word(uint64_t x) const { return x <= half ? x : x + rebase; }
};
// Both at once (lsr_ring_mod_dot_galois_batch): the words of a mod q are fetched through the permutation and lifted,
// the words of b are lifted.  The sign of sigma_g is applied AFTER the lift, against the prime: the lifted word y is the canonical
// residue of the centred v, |v| <= floor(q / 2), and galois_negate(y, p) is the canonical residue of -v, of the same magnitude — the
// operand bound the handle's capacity rests on.  (At an even q the word q / 2 lifts to +q / 2 and its negation is the residue of
// -q / 2, where the materialised sigma_g(a) holds the word q / 2 again, lifted to +q / 2: the two integers differ by q in that
// coefficient, so the integer products differ by a multiple of q, which the reduce removes.)  A clipped word reads 0 and stays 0.
struct LiftGaloisSource {
    static constexpr bool kPermuted = true;
    static constexpr bool kLifted = true;
    GaloisParams g;
    LiftSource lift;
    __device__ __forceinline__ uint32_t lane_product(uint32_t j) const { return j * g.h; }
    __device__ __forceinline__ uint64_t word(uint64_t x) const { return lift.word(x); }
};

template <class A, int LT, bool BHAT, class Src>
__device__ __forceinline__ void tile_ring_dot_from_source(uint64_t* c, const uint64_t* __restrict__ a, const uint64_t* __restrict__ b, size_t total,
                                                          uint32_t nterms, size_t a_os, size_t b_os, uint32_t flags, Src src, ModParams p,
                                                          const typename A::twid* __restrict__ fwd, const typename A::twid* __restrict__ inv,
                                                          RoundConsts<A> cs) {
    __shared__ uint64_t lds[kLdsWords];
    using elem = typename A::elem;
    using twid = typename A::twid;
    constexpr int NR = TileRound<LT, 0>::kCount;
    constexpr int LO0 = TileRound<LT, 0>::LO, R0 = TileRound<LT, 0>::R;               // the mapping the operands are read in
    constexpr int LOL = TileRound<LT, NR - 1>::LO, RL = TileRound<LT, NR - 1>::R;    // the shared last-forward / first-inverse mapping
    constexpr bool kStrided = LT < kTileLog;                                         // several outputs per tile
    constexpr uint32_t kMask = kStrided ? (1u << LT) - 1u : 0xFFFFFFFFu;
    const uint32_t t = threadIdx.x;
    const size_t tile_base = (size_t)blockIdx.x * kTile;
    const uint32_t n = 1u << p.logn;
    const uint32_t nmask = n - 1u;
    const uint32_t block_pos = (uint32_t)(tile_base & nmask);                         // 0: a tile holds whole polynomials
    const size_t left = total - tile_base;
    const uint32_t tile_words = left >= kTile ? kTile : (uint32_t)left;
    const size_t first_output = tile_base >> p.logn;
    const uint32_t outputs = kStrided ? tile_words >> LT : 1u;                        // (total is a multiple of n)
    const rsrc_t out = make_rsrc(c + tile_base, tile_words * 8u);
    const rsrc_t ftab = make_rsrc(fwd, (uint32_t)sizeof(twid) << p.logn);
    const rsrc_t itab = make_rsrc(inv, (uint32_t)sizeof(twid) << p.logn);
    const uint32_t lbase = lane_base<LOL, RL>(t);
    const uint32_t base0 = lane_base<LO0, R0>(t);

    // ntt_tile_ring_dot's operand addressing and clipping of a partial last tile (b)
    auto operand_bytes = [&](uint32_t idx, uint32_t os) -> uint32_t {
        return kStrided ? ((idx & kMask) + (idx >> LT) * os) * 8u : idx * 8u;
    };
    auto operand_words = [&](uint32_t os) -> uint32_t { return kStrided ? (outputs - 1u) * os + n : tile_words; };
    auto operand_word = [&](rsrc_t r, uint32_t os, int k) -> uint64_t {
        const uint32_t reg = reg_offset<LO0, R0>(k);
        const bool present = !kStrided || (base0 >> LT) + (reg >> LT) < outputs;
        const uint64_t raw = buf_load64<kAuxStream>(r, present ? operand_bytes(base0, os) : kRingDotOutOfRange, operand_bytes(reg, os));
        if constexpr (Src::kLifted) return src.word(raw);
        else return raw;
    };
    // Word k of round 0 of a.  kPermuted, sigma_g(a): the same clips, the source word s & (n - 1) of the word's own output, negated
    // where s & n
    const uint32_t lane_jh = src.lane_product(base0 & nmask);
    auto a_word = [&](rsrc_t r, uint32_t os, int k) -> uint64_t {
        if constexpr (Src::kPermuted) {
            const uint32_t reg = reg_offset<LO0, R0>(k);
            const uint32_t output = kStrided ? (base0 >> LT) + (reg >> LT) : 0u;
            const uint32_t s = (lane_jh + (reg & nmask) * src.g.h) & src.g.mask;
            const uint32_t from = kStrided ? ((s & nmask) + output * os) * 8u : (s & nmask) * 8u;
            // (not a streaming load: the eight words of a cache line go to eight different lanes)
            const uint64_t raw = buf_load64(r, output < outputs ? from : kRingDotOutOfRange, 0);
            uint64_t word = raw;
            if constexpr (Src::kLifted) word = src.word(raw);
            return (s & n) ? galois_negate(word, p.q) : word;
        } else {
            return operand_word(r, os, k);
        }
    };
    const uint32_t a_step = (uint32_t)a_os, b_step = (uint32_t)b_os;                  // used when kStrided only: terms n <= 2^27 there
    // first inverse round's twiddles; SKIP_TOP when that round is also the transform's last stage
    auto inverse_first = [&](twid (&slot)[kRoundTwiddles]) {
        load_round_twiddles<A, LOL, RL, true, NR == 1>(slot, lbase, block_pos, nmask, p.logn, itab);
    };
    const uint64_t* a_tile = a + first_output * a_os + block_pos;
    const uint64_t* b_tile = BHAT ? b : b + first_output * b_os + block_pos;

    elem v[kRegs], acc[kRegs];
    twid w[2][kRoundTwiddles];
    constexpr int S1 = BHAT ? NR & 1 : 0;   // twiddle slot of the first inverse round: (S + NR) & 1 of the last forward transform
    if (flags & kRingDotFirst) {
#pragma unroll
        for (int k = 0; k < kRegs; ++k) acc[k] = elem_from_bits<A>(0);
    } else {
#pragma unroll
        for (int k = 0; k < kRegs; ++k) acc[k] = elem_from_bits<A>(buf_load64(out, lbase * 8u, reg_offset<LOL, RL>(k) * 8u));
    }

    for (uint32_t i = 0; i < nterms; ++i, a_tile += n, b_tile += n) {
        const bool last_term = i + 1 == nterms;
        if constexpr (NR > 1) {
            if (i) __syncthreads();                  // the previous term's last LDS reads before this term's first LDS writes
        }
        const rsrc_t ra = make_rsrc(a_tile, operand_words(a_step) * 8u);
        if constexpr (BHAT) {
            ring_forward_tile_from<A, LT, false, 0, false>(v, w, lds, [&](int k) { return a_word(ra, a_step, k); }, ftab, block_pos, nmask, p,
                                                           [&](twid (&slot)[kRoundTwiddles]) {
                                                               if (last_term) inverse_first(slot);
                                                           });
            // b-hat_i at this lane's last-round positions within the polynomial
            const rsrc_t rb = make_rsrc(b_tile, 8u << p.logn);
            const uint32_t lane_off = lbase & kMask;
#pragma unroll
            for (int k = 0; k < kRegs; ++k) {
                const elem bh = A::load(buf_load64(rb, lane_off * 8u, (reg_offset<LOL, RL>(k) & kMask) * 8u), p);
                acc[k] = ring_accumulate<A>(acc[k], ring_product<A>(v[k], bh, p), p);
            }
        } else {
            elem ah[kRegs];
            // a's last round prefetches b's first-round twiddles (round 0 of the same table) into the free slot
            ring_forward_tile_from<A, LT, false, 0, false>(v, w, lds, [&](int k) { return a_word(ra, a_step, k); }, ftab, block_pos, nmask, p,
                                                           [&](twid (&slot)[kRoundTwiddles]) {
                                                               load_round_twiddles<A, LO0, R0, false, false>(slot, base0, block_pos, nmask, p.logn, ftab);
                                                           });
#pragma unroll
            for (int k = 0; k < kRegs; ++k) ah[k] = v[k];
            if constexpr (NR > 1) __syncthreads();   // a's last LDS reads before b's first LDS writes
            const rsrc_t rb = make_rsrc(b_tile, operand_words(b_step) * 8u);
            ring_forward_tile_from<A, LT, false, NR & 1, true>(v, w, lds, [&](int k) { return operand_word(rb, b_step, k); }, ftab, block_pos, nmask, p,
                                                               [&](twid (&slot)[kRoundTwiddles]) {
                                                                   if (last_term) inverse_first(slot);
                                                               });
#pragma unroll
            for (int k = 0; k < kRegs; ++k) acc[k] = ring_accumulate<A>(acc[k], ring_product<A>(ah[k], v[k], p), p);
        }
        if constexpr (std::is_same_v<A, ArithF64>) {
            if ((i & (kRingDotF64Period - 1u)) == kRingDotF64Period - 1u || last_term) {
#pragma unroll
                for (int k = 0; k < kRegs; ++k) acc[k] = recentre_f64(acc[k], p.qd, p.inv_qd);
            }
        }
    }

    if (!(flags & kRingDotLast)) {
#pragma unroll
        for (int k = 0; k < kRegs; ++k) buf_store64(out, lbase * 8u, reg_offset<LOL, RL>(k) * 8u, elem_bits<A>(acc[k]));
        return;
    }
#pragma unroll
    for (int k = 0; k < kRegs; ++k) v[k] = acc[k];

    // inverse rounds (ntt_tile_ring_dot's), the first one straight from registers
    static_for<0, NR>([&](auto ic) {
        constexpr int I = decltype(ic)::value;
        constexpr int J = NR - 1 - I;
        constexpr int LO = TileRound<LT, J>::LO, R = TileRound<LT, J>::R;
        constexpr bool kLast = (I == NR - 1);
        const uint32_t base = lane_base<LO, R>(t);
        uint64_t* const row = lds + lds_slot(base);
        if constexpr (I > 0) {
#pragma unroll
            for (int k = 0; k < kRegs; ++k) v[k] = elem_from_bits<A>(row[lds_slot(reg_offset<LO, R>(k))]);
        }
        if constexpr (!kLast) {
            constexpr int LO1 = TileRound<LT, J - 1>::LO, R1 = TileRound<LT, J - 1>::R;
            load_round_twiddles<A, LO1, R1, true, I + 1 == NR - 1>(w[(S1 + I + 1) & 1], lane_base<LO1, R1>(t), block_pos, nmask, p.logn, itab);
        }
        inverse_round<A, LO, R, kLast>(v, w[(S1 + I) & 1], p, cs);
        if constexpr (kLast) {
#pragma unroll
            for (int k = 0; k < kRegs; ++k) buf_store64<kAuxStream>(out, base * 8u, reg_offset<LO, R>(k) * 8u, A::store_reduced(v[k], p));
        } else {
            constexpr bool kAll = !A::kPartialRecentre;
#pragma unroll
            for (int k = 0; k < kRegs; ++k)
                if (kAll || A::template needs_recentre<R>(k & ((1 << R) - 1))) A::end_of_inverse_round(v[k], p);
            // (I = 0: these are the slots this lane read in the last forward round — no barrier needed before the store)
#pragma unroll
            for (int k = 0; k < kRegs; ++k) row[lds_slot(reg_offset<LO, R>(k))] = elem_bits<A>(v[k]);
            __syncthreads();
        }
    });
}

template <class A, int LT, bool BHAT>
__global__ void __launch_bounds__(kThreads) ntt_tile_ring_dot_galois(uint64_t* c, const uint64_t* __restrict__ a, const uint64_t* __restrict__ b,
                                                                       size_t total, uint32_t nterms, size_t a_os, size_t b_os, uint32_t flags,
                                                                       GaloisParams g, ModParams p, const typename A::twid* __restrict__ fwd,
                                                                       const typename A::twid* __restrict__ inv, RoundConsts<A> cs) {
    tile_ring_dot_from_source<A, LT, BHAT>(c, a, b, total, nterms, a_os, b_os, flags, GaloisSource{g}, p, fwd, inv, cs);
}

// c_j = sum_{i < nterms} a_{j,i} b_{j,i} mod the prime of `p`, where a and b hold words mod ANOTHER modulus q that are centred against q
// and re-based to the prime as they are read (LiftSource): one of the two launches of lsr_ring_mod_dot_batch (lsr_ring_mod.hip).
// Behind the load this is ntt_tile_ring_dot<A, LT, false, BHAT> on the operands lift(a), lift(b), which never exist in memory.  BHAT:
// b holds transforms mod the prime and is read as it is.  An absent output's words read 0, and lift(0) = 0.
template <class A, int LT, bool BHAT>
__global__ void __launch_bounds__(kThreads) ntt_tile_ring_dot_lift(uint64_t* c, const uint64_t* __restrict__ a, const uint64_t* __restrict__ b,
                                                                     size_t total, uint32_t nterms, size_t a_os, size_t b_os, uint32_t flags,
                                                                     LiftSource lift, ModParams p, const typename A::twid* __restrict__ fwd,
                                                                     const typename A::twid* __restrict__ inv, RoundConsts<A> cs) {
    tile_ring_dot_from_source<A, LT, BHAT>(c, a, b, total, nterms, a_os, b_os, flags, lift, p, fwd, inv, cs);
}

// c_j = sum_{i < nterms} sigma_g(a_{j,i}) b_{j,i} mod the prime of `p` on operands mod another modulus q (LiftGaloisSource): one of
// the two launches of lsr_ring_mod_dot_galois_batch (lsr_ring_mod.hip).  Behind the load this is ntt_tile_ring_dot_galois on lift(a),
// lift(b).  BHAT: b holds transforms mod the prime and is read as it is.
template <class A, int LT, bool BHAT>
__global__ void __launch_bounds__(kThreads) ntt_tile_ring_dot_lift_galois(uint64_t* c, const uint64_t* __restrict__ a, const uint64_t* __restrict__ b,
                                                                            size_t total, uint32_t nterms, size_t a_os, size_t b_os, uint32_t flags,
                                                                            GaloisParams g, LiftSource lift, ModParams p,
                                                                            const typename A::twid* __restrict__ fwd,
                                                                            const typename A::twid* __restrict__ inv, RoundConsts<A> cs) {
    tile_ring_dot_from_source<A, LT, BHAT>(c, a, b, total, nterms, a_os, b_os, flags, LiftGaloisSource{g, lift}, p, fwd, inv, cs);
}

}  // namespace lsr
