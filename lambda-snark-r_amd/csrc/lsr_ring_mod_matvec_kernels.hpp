// y = M x and y = M G^-1(x) under an arbitrary modulus q in the tile (lsr_ring_mod_matvec.hip): ntt_tile_ring_matvec
// and ntt_tile_ring_matvec_gadget (lsr_ring_matvec_kernels.hpp, lsr_ring_gadget_kernels.hpp) with three differences.
//   Loader        x holds words mod q.  Plain: the word goes through LiftSource::word, the residue mod the launch's prime of its
//                 centred representative.  Gadget: digit d of the word, extracted against q, as its residue mod the launch's prime.
//                 A word a ragged tile clips reads 0, which both forms map to 0.
//   Column range  the launch covers matrix columns [col0, col0 + ncols) of a matrix whose rows lie m_row_words apart; y holds `rows`
//                 rows per vector.  A gadget range may begin and end between two digits of one column of x.
//   Both primes   grid z is the prime: everything that depends on it comes as a two-element array indexed by blockIdx.z, which is
//                 wave-uniform, so the loads behind the index are scalar.
//   Check         (CHECK, the plain form only: lsr_ring_mod_matvec_bounded_batch) ahead of each column's load stage the
//                 checking workgroup takes the column's words — the loader's addresses, sixteen loads in flight — and holds them
//                 against q and against the caller's bound, by sign bits of differences as ntt_tile_ring_mod_fold does.  A tile
//                 spans several vectors of the batch — register k of a lane belongs to vector first_vector + (base0 >> LT) +
//                 (reg_offset(k) >> LT) — so there is no wave-wide OR: a lane keeps one "over the bound" and one ">= q" bit PER
//                 REGISTER in one 32-bit mask over the column loop, and behind the loop ORs the set bits, and only those, into the
//                 flag word of the vector that owns the register.  Clean operands cost no atomic.  A clipped word reads 0 and
//                 passes; a lane whose vector is absent touches no flag word.  One workgroup per tile checks: prime 0, row block 0.
// Behind the load, the instruction sequence, the barriers and the FP64 re-centring period are the single-prime kernels'.  The output
// is one prime's inverse-transformed sums; the reduce pass (lsr_ring_mod_kernels.hpp) joins the two.
#pragma once

#include "lsr_ring_gadget_digits.hpp"
#include "lsr_ring_mod_kernels.hpp"

namespace lsr {

// what one prime brings to a launch
template <class A>
struct RingModMatvecPrime {
    uint64_t* y;                       // [vectors][rows][n]: this prime's sums
    const uint64_t* mhat;              // M-hat of this prime at [first row of the launch][0]
    const typename A::twid* fwd;
    const typename A::twid* inv;
    ModParams p;
    RoundConsts<A> cs;
    LiftSource lift;
};
template <class A>
struct RingModMatvecPrimes {
    RingModMatvecPrime<A> prime[2];
};

// x: [batch][xcols][n] words mod q (plain: xcols = the matrix's columns; gadget: the matrix has xcols digits columns).  `total` =
// vectors n words of the batch axis.  Grid: x = tile of the batch axis, y = row block, z = prime (1 or 2 entries of `both` in use).
// Operand addressing and ranges: ntt_tile_ring_matvec's, with xcols n words between consecutive vectors' columns of x and rows n
// between their rows of y.  CHECK: vec_flags holds one flag word per vector of the launch (the bits of ring_mod_gram_lift_kernel), and a
// word x < q passes when its centred magnitude min(x, q - x) <= bound; without CHECK neither is read.
template <class A, int LT, int RB, bool GADGET, bool BOTH, bool CHECK = false>
__global__ void __launch_bounds__(kThreads) ntt_tile_ring_mod_matvec(RingModMatvecPrimes<A> both, const uint64_t* __restrict__ x, size_t total, uint32_t rows,
                                                                       uint32_t xcols, uint32_t col0, uint32_t ncols, size_t m_row_words, uint64_t q,
                                                                       GadgetParams g, uint32_t* __restrict__ vec_flags = nullptr, uint64_t bound = 0) {
    static_assert(!CHECK || (BOTH && !GADGET), "the check belongs to the plain product, both primes in one launch");
    __shared__ uint64_t lds[kLdsWords];
    using elem = typename A::elem;
    using twid = typename A::twid;
    constexpr int NR = TileRound<LT, 0>::kCount;
    constexpr int LO0 = TileRound<LT, 0>::LO, R0 = TileRound<LT, 0>::R;               // the mapping x is read and y is written in
    constexpr int LOL = TileRound<LT, NR - 1>::LO, RL = TileRound<LT, NR - 1>::R;    // the shared last-forward / first-inverse mapping
    constexpr bool kStrided = LT < kTileLog;                                         // several vectors per tile
    constexpr uint32_t kMask = kStrided ? (1u << LT) - 1u : 0xFFFFFFFFu;
    constexpr int S1 = NR & 1;                                                       // twiddle slot of the first inverse round
    const RingModMatvecPrime<A>& mine = both.prime[BOTH ? blockIdx.z : 0u];          // wave-uniform: kernel arguments at a scalar offset
    const ModParams p = mine.p;
    const RoundConsts<A> cs = mine.cs;
    const LiftSource lift = mine.lift;
    uint64_t* const y = mine.y;
    const uint64_t* const mhat = mine.mhat;
    const uint32_t t = threadIdx.x;
    const size_t tile_base = (size_t)blockIdx.x * kTile;
    const uint32_t n = 1u << p.logn;
    const uint32_t nmask = n - 1u;
    const uint32_t block_pos = (uint32_t)(tile_base & nmask);
    const size_t left = total - tile_base;
    const uint32_t tile_words = left >= kTile ? kTile : (uint32_t)left;
    const size_t first_vector = tile_base >> p.logn;
    const uint32_t vectors = kStrided ? tile_words >> LT : 1u;                        // (total is a multiple of n)
    const uint32_t row0 = blockIdx.y * RB;
    const uint32_t nrows = rows - row0 < (uint32_t)RB ? rows - row0 : (uint32_t)RB;   // workgroup-uniform
    const rsrc_t ftab = make_rsrc(mine.fwd, (uint32_t)sizeof(twid) << p.logn);
    const rsrc_t itab = make_rsrc(mine.inv, (uint32_t)sizeof(twid) << p.logn);
    const uint32_t lbase = lane_base<LOL, RL>(t);
    const uint32_t base0 = lane_base<LO0, R0>(t);
    const uint32_t x_step = xcols * n, y_step = rows * n;                             // used when kStrided only: below 2^28 there

    // ntt_tile_ring_matvec's operand addressing and clipping of a partial last tile
    auto operand_bytes = [&](uint32_t idx, uint32_t os) -> uint32_t {
        return kStrided ? ((idx & kMask) + (idx >> LT) * os) * 8u : idx * 8u;
    };
    auto operand_words = [&](uint32_t os) -> uint32_t { return kStrided ? (vectors - 1u) * os + n : tile_words; };
    auto lane_bytes = [&](uint32_t reg, uint32_t os) -> uint32_t {
        const bool present = !kStrided || (base0 >> LT) + (reg >> LT) < vectors;
        return present ? operand_bytes(base0, os) : kRingDotOutOfRange;
    };
    auto inverse_first = [&](twid (&slot)[kRoundTwiddles]) {
        load_round_twiddles<A, LOL, RL, true, NR == 1>(slot, lbase, block_pos, nmask, p.logn, itab);
    };

    elem v[kRegs], acc[RB][kRegs];
    twid w[2][kRoundTwiddles];
    // CHECK: bit k: some word of register k was over the bound; bit 16 + k: some word of register k was >= q (which -1 overrides)
    static_assert(kRegs == 16, "one violation mask holds two bits per register");
    const bool check = CHECK && blockIdx.z == 0 && blockIdx.y == 0;                   // workgroup-uniform: the other workgroups of the tile read the same words
    const uint64_t upper = q - bound;         // the centred magnitude of a word below q exceeds the bound between bound and q - bound
    uint32_t violations = 0;
#pragma unroll
    for (int r = 0; r < RB; ++r) {
#pragma unroll
        for (int k = 0; k < kRegs; ++k) acc[r][k] = elem_from_bits<A>(0);
    }

    // matrix column c reads column xc of x: c itself, or (gadget) c = xc D + d and digit d of it
    uint32_t xc = GADGET ? col0 / g.digits : col0;
    uint32_t d = GADGET ? col0 - xc * g.digits : 0u;
    const uint64_t* x_tile = x + (first_vector * xcols + xc) * n + block_pos;
    const uint64_t* m_col = mhat + (size_t)row0 * m_row_words + (size_t)col0 * n;     // M-hat[row0][c]; row r of the block: + r m_row_words
    const uint32_t m_lane = (lbase & kMask) * 8u;
    for (uint32_t i = 0; i < ncols; ++i, m_col += n) {
        const bool last_col = i + 1 == ncols;
        if constexpr (NR > 1) {
            if (i) __syncthreads();                  // the previous column's last LDS reads before this column's first LDS writes
        }
        const rsrc_t rx = make_rsrc(x_tile, operand_words(x_step) * 8u);
        const uint32_t shift = d * g.base_log2;
        if constexpr (CHECK) {
            // The checking workgroup takes the column's words once more, ahead of the load stage that lifts them (the second read
            // is served by the cache), sixteen loads in flight and then arithmetic alone.  With the check inside the loader, a uniform
            // branch per register, n = 64, 16 x 256, batch 1024 measured 1608 us against 1345 this way (the plain product: 1208).
            if (check) {
                uint64_t word[kRegs];
#pragma unroll
                for (int k = 0; k < kRegs; ++k) {
                    const uint32_t reg = reg_offset<LO0, R0>(k);
                    word[k] = buf_load64(rx, lane_bytes(reg, x_step), operand_bytes(reg, x_step));
                }
#pragma unroll
                for (int k = 0; k < kRegs; ++k) {
                    // sign bits of differences instead of compares, as in ntt_tile_ring_mod_fold: q, the bound and q - bound are below
                    // 2^63, so for a word below 2^63 bit 63 of x - y says x < y; a word at or above 2^63 is >= q by its own bit 63.
                    // 0, what a clipped word reads, passes both.
                    const uint32_t not_below_q = ~(uint32_t)((word[k] - q) >> 32) | (uint32_t)(word[k] >> 32);
                    const uint32_t over_bound = (uint32_t)((bound - word[k]) >> 32) & (uint32_t)((word[k] - upper) >> 32);   // bound < word < q - bound
                    violations |= ((over_bound >> 31) << k) | ((not_below_q >> 31) << (16 + k));
                }
            }
        }
        ring_forward_tile_from<A, LT, false, 0, false>(
            v, w, lds,
            [&](int k) {
                const uint32_t reg = reg_offset<LO0, R0>(k);
                if constexpr (GADGET) {
                    // (not a streaming load: the same words come back for the next digit and for the other prime)
                    return gadget_digit(gadget_shifted(buf_load64(rx, lane_bytes(reg, x_step), operand_bytes(reg, x_step)), q, g), shift, p.q, g);
                } else {
                    return lift.word(buf_load64(rx, lane_bytes(reg, x_step), operand_bytes(reg, x_step)));
                }
            },
            ftab, block_pos, nmask, p,
            [&](twid (&slot)[kRoundTwiddles]) {
                if (last_col) inverse_first(slot);
            });
        static_for<0, RB>([&](auto rc) {
            constexpr int r = decltype(rc)::value;
            if ((uint32_t)r < nrows) {
                const rsrc_t rm = make_rsrc(m_col + r * m_row_words, 8u << p.logn);
#pragma unroll
                for (int k = 0; k < kRegs; ++k) {
                    const elem mh = A::load(buf_load64(rm, m_lane, (reg_offset<LOL, RL>(k) & kMask) * 8u), p);
                    acc[r][k] = ring_accumulate<A>(acc[r][k], ring_product<A>(v[k], mh, p), p);
                }
            }
        });
        if constexpr (std::is_same_v<A, ArithF64>) {
            if ((i & (kRingDotF64Period - 1u)) == kRingDotF64Period - 1u || last_col) {
#pragma unroll
                for (int r = 0; r < RB; ++r) {
#pragma unroll
                    for (int k = 0; k < kRegs; ++k) acc[r][k] = recentre_f64(acc[r][k], p.qd, p.inv_qd);
                }
            }
        }
        if constexpr (GADGET) {
            if (++d == g.digits) {                   // workgroup-uniform
                d = 0;
                x_tile += n;
            }
        } else {
            x_tile += n;
        }
    }

    if constexpr (CHECK) {
        // the rare path: a lane that saw a violation tells the vector that owns the register, and no other
        if (check && violations) {
#pragma unroll
            for (int k = 0; k < kRegs; ++k) {
                const uint32_t reg = reg_offset<LO0, R0>(k);
                const uint32_t bits = ((violations >> k) & 1u ? kGramFlagOverBound : 0u) | ((violations >> (16 + k)) & 1u ? kGramFlagNotBelowQ : 0u);
                const uint32_t in_tile = kStrided ? (base0 >> LT) + (reg >> LT) : 0u;
                if (bits && in_tile < vectors) atomicOr(&vec_flags[first_vector + in_tile], bits);   // (in_tile < vectors: the lane's vector is present)
            }
        }
    }

    // per row the inverse rounds (ntt_tile_ring_matvec's), the first one straight from the accumulator
    static_for<0, RB>([&](auto rc) {
        constexpr int r = decltype(rc)::value;
        if ((uint32_t)r >= nrows) return;
        if constexpr (r > 0) {
            if constexpr (NR > 1) __syncthreads();   // the previous row's last LDS reads before this row's first LDS writes
            inverse_first(w[S1]);                    // (row 0 got them under the last column's last forward round)
        }
        const uint64_t* y_tile = y + (first_vector * rows + row0 + r) * n + block_pos;
        const rsrc_t out = make_rsrc(y_tile, operand_words(y_step) * 8u);
#pragma unroll
        for (int k = 0; k < kRegs; ++k) v[k] = acc[r][k];
        static_for<0, NR>([&](auto ic) {
            constexpr int I = decltype(ic)::value;
            constexpr int J = NR - 1 - I;
            constexpr int LO = TileRound<LT, J>::LO, R = TileRound<LT, J>::R;
            constexpr bool kLast = (I == NR - 1);
            uint64_t* const row = lds + lds_slot(lane_base<LO, R>(t));
            if constexpr (I > 0) {
#pragma unroll
                for (int k = 0; k < kRegs; ++k) v[k] = elem_from_bits<A>(row[lds_slot(reg_offset<LO, R>(k))]);
            }
            if constexpr (!kLast) {
                constexpr int LO1 = TileRound<LT, J - 1>::LO, R1 = TileRound<LT, J - 1>::R;
                load_round_twiddles<A, LO1, R1, true, I + 1 == NR - 1>(w[(S1 + I + 1) & 1], lane_base<LO1, R1>(t), block_pos, nmask, p.logn, itab);
            }
            inverse_round<A, LO, R, kLast>(v, w[(S1 + I) & 1], p, cs);
            if constexpr (kLast) {               // J = 0: the mapping (LO0, R0)
#pragma unroll
                for (int k = 0; k < kRegs; ++k) {
                    const uint32_t reg = reg_offset<LO0, R0>(k);
                    buf_store64<kAuxStream>(out, lane_bytes(reg, y_step), operand_bytes(reg, y_step), A::store_reduced(v[k], p));
                }
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
    });
}

}  // namespace lsr
