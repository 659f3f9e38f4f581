// Ring matrix-vector product y_j = M x_j in the tile (lsr_ring_matvec.hip): ntt_tile_ring_dot's shared-b form
// (lsr_ntt_kernels.hpp) with RB accumulators.  One workgroup owns one 4096-word tile of the batch axis and one block of up to RB
// rows of M.  Per column c it runs the forward rounds of its tile of x[.][c] ONCE and, for each row r of the block, multiplies the
// result by M-hat[r][c] (read at the last-round positions, as a shared b-hat) into that row's 16 accumulator registers.  After the
// last column the rows' inverse transforms run one after the other through the one LDS tile, each stored to y[.][r].
#pragma once

#include "lsr_ntt_kernels.hpp"

namespace lsr {

// y: [batch][rows][n]; x: [batch][cols][n] (both natural order, canonical); mhat: [rows][cols][n], each polynomial the canonical
// forward transform in the order launch_ntt writes.  `total` = batch n words: the extent of the batch axis, tiled as ring_dot tiles
// its output.  Grid: x = tile of the batch axis, y = row block.
// Operand addressing (ntt_tile_ring_dot's): the words of x[j][c] are n contiguous words, consecutive vectors' column-c polynomials
// lie cols n words apart; y[j][r] likewise with rows n.  A tile index idx = vector (idx >> LT) | coefficient (idx & (n - 1)) splits
// into a lane part and a workgroup-uniform register part in every round mapping.  Ranges: x of one tile spans at most 4096 cols
// words, y at most 4096 rows words — below 2^31 bytes by LSR_RING_DOT_MAX_TERMS and LSR_RING_MATVEC_MAX_ROWS; M-hat is addressed
// one polynomial at a time from a 64-bit pointer.
// Accumulator contract: ring_dot's, per row (the rows' accumulators never meet).
template <class A, int LT, int RB>
__global__ void __launch_bounds__(kThreads) ntt_tile_ring_matvec(uint64_t* __restrict__ y, const uint64_t* __restrict__ x, const uint64_t* __restrict__ mhat,
                                                                   size_t total, uint32_t rows, uint32_t cols, ModParams p,
                                                                   const typename A::twid* __restrict__ fwd, const typename A::twid* __restrict__ inv,
                                                                   RoundConsts<A> cs) {
    __shared__ uint64_t lds[kLdsWords];
    using elem = typename A::elem;
    using twid = typename A::twid;
    constexpr int NR = TileRound<LT, 0>::kCount;
    constexpr int LO0 = TileRound<LT, 0>::LO, R0 = TileRound<LT, 0>::R;               // the mapping x is read and y is written in
    constexpr int LOL = TileRound<LT, NR - 1>::LO, RL = TileRound<LT, NR - 1>::R;    // the shared last-forward / first-inverse mapping
    constexpr bool kStrided = LT < kTileLog;                                         // several vectors per tile
    constexpr uint32_t kMask = kStrided ? (1u << LT) - 1u : 0xFFFFFFFFu;
    constexpr int S1 = NR & 1;                                                       // twiddle slot of the first inverse round
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
    const rsrc_t ftab = make_rsrc(fwd, (uint32_t)sizeof(twid) << p.logn);
    const rsrc_t itab = make_rsrc(inv, (uint32_t)sizeof(twid) << p.logn);
    const uint32_t lbase = lane_base<LOL, RL>(t);
    const uint32_t base0 = lane_base<LO0, R0>(t);
    const uint32_t x_step = cols * n, y_step = rows * n;                              // used when kStrided only: below 2^28 there

    // ntt_tile_ring_dot's operand addressing: byte offset of tile index part `idx` where vectors lie `os` words apart; a partial
    // last tile is clipped by the range of the buffer resource and by an out-of-range lane offset for a vector the tile does not have
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
#pragma unroll
    for (int r = 0; r < RB; ++r) {
#pragma unroll
        for (int k = 0; k < kRegs; ++k) acc[r][k] = elem_from_bits<A>(0);
    }

    const uint64_t* x_tile = x + first_vector * cols * n + block_pos;
    const uint64_t* m_col = mhat + (size_t)row0 * cols * n;                           // M-hat[row0][c]; row r of the block: + r cols n
    const size_t m_row_words = (size_t)cols * n;
    const uint32_t m_lane = (lbase & kMask) * 8u;
    for (uint32_t c = 0; c < cols; ++c, x_tile += n, m_col += n) {
        const bool last_col = c + 1 == cols;
        if constexpr (NR > 1) {
            if (c) __syncthreads();                  // the previous column's last LDS reads before this column's first LDS writes
        }
        const rsrc_t rx = make_rsrc(x_tile, operand_words(x_step) * 8u);
        ring_forward_tile_from<A, LT, false, 0, false>(
            v, w, lds,
            [&](int k) {
                const uint32_t reg = reg_offset<LO0, R0>(k);
                return buf_load64<kAuxStream>(rx, lane_bytes(reg, x_step), operand_bytes(reg, x_step));
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
            if ((c & (kRingDotF64Period - 1u)) == kRingDotF64Period - 1u || last_col) {
#pragma unroll
                for (int r = 0; r < RB; ++r) {
#pragma unroll
                    for (int k = 0; k < kRegs; ++k) acc[r][k] = recentre_f64(acc[r][k], p.qd, p.inv_qd);
                }
            }
        }
    }

    // per row the inverse rounds (ntt_tile_ring_dot's schedule), the first one straight from the accumulator
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
