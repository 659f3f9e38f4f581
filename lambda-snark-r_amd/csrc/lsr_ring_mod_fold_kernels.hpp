// Fold of ring vectors by ring-valued challenges under an arbitrary modulus q in the tile (lsr_ring_mod_fold.hip, batch.h "fold under
// any modulus"):
//   z[j][c] = sum_{i < terms} p[j][i] * v[j term_stride + i][c]   over the integers, mod one of the handle's two NTT primes.
// ntt_tile_ring_fold<A, LT, false> (lsr_ring_fold_kernels.hpp) with the load stage of ntt_tile_ring_dot_lift
// (lsr_ring_galois_kernels.hpp) and a check in it:
//   Loader   v holds words mod q.  A word goes through LiftSource::word — the residue mod the launch's prime of its centred
//            representative — as it is loaded; lifted copies of v never exist in memory.  A word the ragged last tile clips reads 0,
//            and lift(0) = 0.
//   Check    the same word is held against q and against bound_v: "over the bound" / ">= q" are collected per lane over all terms,
//            OR-ed across the wave by ballot, and at most one atomic OR per wave goes to the output's flag word (the bits and the
//            flag layout of ring_mod_gram_lift_kernel, lsr_ring_mod_kernels.hpp).  Only one prime's workgroups check: the
//            other prime reads the same words.
//   Output   the launch's sums are complete (a group of terms is one whole sum: the groups are joined mod q by the reduce pass, not
//            in the accumulator), so there is no kRingDotFirst / kRingDotLast hand-over.
//   Primes   both in one launch, the prime as grid z: everything that depends on it comes as a two-element kernel argument indexed
//            by blockIdx.z, which is wave-uniform, and the workgroups of prime 0 check (a uniform branch around sign-bit arithmetic
//            on the loaded words — no lane masks kept).  In this form the kernel stays within 14 VGPRs of ntt_tile_ring_fold
//            and keeps its occupancy but for n = 2 in the FP64 flavour (4 waves per SIMD against 5); one launch per prime with the check
//            as a template argument cost the checking launch 20 to 34 VGPRs in the FP64 flavour, spilled SGPRs, and a wave at most sizes
//            (profiles/r35_ring_mod_fold_resource_usage.txt).
// Grid x and y, operand addressing, buffer-resource clipping of the ragged tile, barriers and the FP64 re-centring period are the fold
// kernel's.  Accumulator contract: the fold kernel's, unchanged — a lifted word below q is a canonical residue of the prime.  (A word
// >= q may lift to anything: its output is flagged and the reduce pass writes zeros over whatever the sums hold.)
#pragma once

#include "lsr_ring_mod_kernels.hpp"

namespace lsr {

// what one prime brings to a launch
template <class A>
struct RingModFoldPrime {
    uint64_t* sums;                    // [outputs][total]: this prime's inverse-transformed sums
    const uint64_t* bhat;              // [outputs][nterms][n]: the transforms of the lifted challenges, as launch_ntt writes them
    const typename A::twid* fwd;
    const typename A::twid* inv;
    ModParams p;
    RoundConsts<A> cs;
    LiftSource lift;
};
template <class A>
struct RingModFoldPrimes {
    RingModFoldPrime<A> prime[2];
};

// what both primes of a launch share
struct RingModFoldShape {
    size_t total;            // words of one output: width n
    uint32_t nterms;
    size_t a_term, a_out;    // words between consecutive terms / consecutive outputs' first terms in v
    uint64_t q, bound;       // a word x < q passes when its centred magnitude min(x, q - x) <= bound
};

// a: term i of output j at a + j a_out + i a_term, `total` contiguous words mod q.  Grid: x = tiles of the [width][n] words of one
// output, y = output, z = prime.
template <class A, int LT>
__global__ void __launch_bounds__(kThreads) ntt_tile_ring_mod_fold(RingModFoldPrimes<A> both, const uint64_t* __restrict__ a, uint32_t* __restrict__ out_flags,
                                                                     RingModFoldShape s) {
    const RingModFoldPrime<A>& mine = both.prime[blockIdx.z];   // wave-uniform: kernel arguments at a scalar offset
    const bool check = blockIdx.z == 0;                          // workgroup-uniform
    __shared__ uint64_t lds[kLdsWords];
    using elem = typename A::elem;
    using twid = typename A::twid;
    constexpr int NR = TileRound<LT, 0>::kCount;
    constexpr int LO0 = TileRound<LT, 0>::LO, R0 = TileRound<LT, 0>::R;               // the mapping the operands are read in
    constexpr int LOL = TileRound<LT, NR - 1>::LO, RL = TileRound<LT, NR - 1>::R;    // the shared last-forward / first-inverse mapping
    constexpr uint32_t kMask = LT < kTileLog ? (1u << LT) - 1u : 0xFFFFFFFFu;        // several components per tile
    constexpr int S1 = NR & 1;                                                       // twiddle slot of the first inverse round
    const ModParams p = mine.p;
    const RoundConsts<A> cs = mine.cs;
    const LiftSource lift = mine.lift;
    const uint32_t t = threadIdx.x;
    const size_t j = blockIdx.y;
    const size_t tile_base = (size_t)blockIdx.x * kTile;
    const uint32_t n = 1u << p.logn;
    const uint32_t nmask = n - 1u;
    const uint32_t block_pos = (uint32_t)(tile_base & nmask);
    const size_t left = s.total - tile_base;
    const uint32_t tile_bytes = (left >= kTile ? kTile : (uint32_t)left) * 8u;
    const rsrc_t out = make_rsrc(mine.sums + j * s.total + tile_base, tile_bytes);
    const rsrc_t ftab = make_rsrc(mine.fwd, (uint32_t)sizeof(twid) << p.logn);
    const rsrc_t itab = make_rsrc(mine.inv, (uint32_t)sizeof(twid) << p.logn);
    const uint32_t lbase = lane_base<LOL, RL>(t);
    const uint32_t base0 = lane_base<LO0, R0>(t);
    // first inverse round's twiddles; SKIP_TOP when that round is also the transform's last stage
    auto inverse_first = [&](twid (&slot)[kRoundTwiddles]) {
        load_round_twiddles<A, LOL, RL, true, NR == 1>(slot, lbase, block_pos, nmask, p.logn, itab);
    };
    const uint64_t* a_tile = a + j * s.a_out + tile_base;
    const uint64_t* b_tile = mine.bhat + j * ((size_t)s.nterms << p.logn);
    const uint32_t b_lane = (lbase & kMask) * 8u;

    elem v[kRegs], acc[kRegs];
    twid w[2][kRoundTwiddles];
    const uint64_t upper = s.q - s.bound;     // the centred magnitude of a word below q exceeds the bound between bound and q - bound
    uint32_t not_below_q = 0, over_bound = 0;   // bit 31: some word of this lane was >= q / over the bound (which -1 overrides)
#pragma unroll
    for (int k = 0; k < kRegs; ++k) acc[k] = elem_from_bits<A>(0);

    for (uint32_t i = 0; i < s.nterms; ++i, a_tile += s.a_term, b_tile += n) {
        const bool last_term = i + 1 == s.nterms;
        if constexpr (NR > 1) {
            if (i) __syncthreads();                  // the previous term's last LDS reads before this term's first LDS writes
        }
        const rsrc_t ra = make_rsrc(a_tile, tile_bytes);
        ring_forward_tile_from<A, LT, false, 0, false>(
            v, w, lds,
            [&](int k) {
                const uint64_t word = buf_load64<kAuxStream>(ra, base0 * 8u, reg_offset<LO0, R0>(k) * 8u);
                if (check) {
                    // sign bits of differences instead of compares: no lane masks to keep.  q, the bound and q - bound are below
                    // 2^63, so for a word below 2^63 bit 63 of x - y says x < y; a word at or above 2^63 is >= q by its own bit 63.
                    not_below_q |= ~(uint32_t)((word - s.q) >> 32) | (uint32_t)(word >> 32);
                    over_bound |= (uint32_t)((s.bound - word) >> 32) & (uint32_t)((word - upper) >> 32);   // bound < word < q - bound
                }
                return lift.word(word);
            },
            ftab, block_pos, nmask, p,
            [&](twid (&slot)[kRoundTwiddles]) {
                if (last_term) inverse_first(slot);
            });
        // b-hat_i at this lane's last-round positions within the polynomial
        const rsrc_t rb = make_rsrc(b_tile, 8u << p.logn);
#pragma unroll
        for (int k = 0; k < kRegs; ++k) {
            const elem bh = A::load(buf_load64(rb, b_lane, (reg_offset<LOL, RL>(k) & kMask) * 8u), p);
            acc[k] = ring_accumulate<A>(acc[k], ring_product<A>(v[k], bh, p), p);
        }
        if constexpr (std::is_same_v<A, ArithF64>) {
            if ((i & (kRingDotF64Period - 1u)) == kRingDotF64Period - 1u || last_term) {
#pragma unroll
                for (int k = 0; k < kRegs; ++k) acc[k] = recentre_f64(acc[k], p.qd, p.inv_qd);
            }
        }
    }

    if (check) {
        // every lane of the workgroup arrives here: the ballots see whole waves
        const uint32_t wave_bits = (__ballot(over_bound >> 31) ? kGramFlagOverBound : 0u) | (__ballot(not_below_q >> 31) ? kGramFlagNotBelowQ : 0u);
        if (wave_bits && (t & (warpSize - 1)) == 0) atomicOr(&out_flags[j], wave_bits);
    }
#pragma unroll
    for (int k = 0; k < kRegs; ++k) v[k] = acc[k];

    // inverse rounds (ntt_tile_ring_fold's schedule), the first one straight from registers
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

}  // namespace lsr
