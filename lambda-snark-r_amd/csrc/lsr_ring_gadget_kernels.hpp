// Gadget decomposition of ring elements (lsr_ring_gadget.hip, batch.h): balanced base-2^b digits without a carry chain,
// their recomposition, the l-infinity norm, and y = M G^-1(x) with the digits extracted in the load stage of the mat-vec's tile kernel.
#pragma once

#include "lsr_ring_gadget_digits.hpp"
#include "lsr_ring_matvec_kernels.hpp"

namespace lsr {

// (GadgetParams, gadget_shifted and gadget_digit: lsr_ring_gadget_digits.hpp)

// out[j][d][k] = digit d of x[j][k]; `total` = count n words of x.  Each word is read once; its D digits leave from registers, each
// store instruction of a wave covering 64 consecutive words of one digit polynomial.
__global__ void __launch_bounds__(kThreads) ring_decompose_kernel(uint64_t* __restrict__ out, const uint64_t* __restrict__ x, size_t total, int logn,
                                                                    uint64_t q, GadgetParams g) {
    const size_t nmask = ((size_t)1 << logn) - 1;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
        const uint64_t u = gadget_shifted(x[i], q, g);
        uint64_t* o = out + (((i >> logn) * g.digits) << logn) + (i & nmask);
        for (uint32_t d = 0, shift = 0; d < g.digits; ++d, shift += g.base_log2, o += nmask + 1) *o = gadget_digit(u, shift, q, g);
    }
}

// B^d mod q for d < D, computed on the host (D <= 33: b (D - 1) <= 64 and b >= 2)
constexpr int kGadgetMaxDigits = 33;
struct GadgetPowers {
    uint64_t pw[kGadgetMaxDigits];
};

// out[j][k] = sum_d B^d z[j][d][k] mod q for canonical z.  GOLD: q = 2^64 - 2^32 + 1 (above the Barrett product's 2^61 limit).
template <bool GOLD>
__global__ void __launch_bounds__(kThreads) ring_recompose_kernel(uint64_t* __restrict__ out, const uint64_t* __restrict__ z, size_t total, int logn,
                                                                    uint32_t digits, ModParams p, GadgetPowers w) {
    const size_t nmask = ((size_t)1 << logn) - 1;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
        const uint64_t* src = z + (((i >> logn) * digits) << logn) + (i & nmask);
        uint64_t acc = 0;
        for (uint32_t d = 0; d < digits; ++d, src += nmask + 1) {
            if constexpr (GOLD) {
                acc = gold_add(acc, gold_mul(*src, w.pw[d]));
            } else {
                const uint64_t s = acc + mulmod_barrett128(*src, w.pw[d], p);   // both canonical: below 2 q < 2^62
                acc = s >= p.q ? s - p.q : s;
            }
        }
        out[i] = acc;
    }
}

// linf[j] = max_k |centred x[j][k]|, or UINT64_MAX when a word of element j is not below q.  One workgroup of blockDim.x lanes (a
// multiple of 64, at most kThreads) per element: per-lane maximum, wave reduction, the waves' maxima through LDS, one plain store.
__global__ void __launch_bounds__(kThreads) ring_linf_kernel(uint64_t* __restrict__ linf, const uint64_t* __restrict__ x, size_t count, int logn, uint64_t q) {
    __shared__ uint64_t wave_max[kThreads / 64];
    const uint64_t half_q = q >> 1;
    const uint32_t n = 1u << logn, t = threadIdx.x, waves = blockDim.x / 64;
    for (size_t j = blockIdx.x; j < count; j += gridDim.x) {
        const uint64_t* e = x + (j << logn);
        uint64_t m = 0;
        for (uint32_t k = t; k < n; k += blockDim.x) {
            const uint64_t v = e[k];
            const uint64_t a = v >= q ? ~0ull : v > half_q ? q - v : v;
            m = a > m ? a : m;
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            const uint64_t other = __shfl_xor((unsigned long long)m, s, 64);
            m = other > m ? other : m;
        }
        if ((t & 63u) == 0) wave_max[t >> 6] = m;
        __syncthreads();
        if (t == 0) {
            for (uint32_t w = 1; w < waves; ++w) m = wave_max[w] > m ? wave_max[w] : m;
            linf[j] = m;
        }
        __syncthreads();   // wave_max is written again for the workgroup's next element
    }
}

// y = M G^-1(x): ntt_tile_ring_matvec (lsr_ring_matvec_kernels.hpp) with the column loop running over (xc, d), matrix column
// c = xc D + d.  x: [batch][xcols][n]; y, mhat, total and the grid as there; cols = xcols D.  The loader handed to
// ring_forward_tile_from reads the word of x[.][xc] the plain kernel would read from column c of a decomposed vector and returns
// digit d of it as the canonical word, so everything behind the load is the plain kernel's instruction sequence on the plain
// kernel's operands: y equals matvec(decompose(x)) word for word.  A word a ragged tile clips reads as 0, whose digits are 0.
// The tile of x[.][xc] is fetched once per digit; after the first time it comes from L2 (16 words per lane held across the digits
// would cost 32 VGPRs the F64 and Gold instantiations at LT = 12 do not have: they sit at 256).
template <class A, int LT, int RB>
__global__ void __launch_bounds__(kThreads) ntt_tile_ring_matvec_gadget(uint64_t* __restrict__ y, const uint64_t* __restrict__ x,
                                                                          const uint64_t* __restrict__ mhat, size_t total, uint32_t rows, uint32_t xcols,
                                                                          GadgetParams g, ModParams p, const typename A::twid* __restrict__ fwd,
                                                                          const typename A::twid* __restrict__ inv, RoundConsts<A> cs) {
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
    const uint32_t cols = xcols * g.digits;
    const rsrc_t ftab = make_rsrc(fwd, (uint32_t)sizeof(twid) << p.logn);
    const rsrc_t itab = make_rsrc(inv, (uint32_t)sizeof(twid) << p.logn);
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
#pragma unroll
    for (int r = 0; r < RB; ++r) {
#pragma unroll
        for (int k = 0; k < kRegs; ++k) acc[r][k] = elem_from_bits<A>(0);
    }

    const uint64_t* x_tile = x + first_vector * xcols * n + block_pos;
    const uint64_t* m_col = mhat + (size_t)row0 * cols * n;                           // M-hat[row0][c]; row r of the block: + r cols n
    const size_t m_row_words = (size_t)cols * n;
    const uint32_t m_lane = (lbase & kMask) * 8u;
    uint32_t c = 0;
    for (uint32_t xc = 0; xc < xcols; ++xc, x_tile += n) {
        const rsrc_t rx = make_rsrc(x_tile, operand_words(x_step) * 8u);
        for (uint32_t d = 0, shift = 0; d < g.digits; ++d, shift += g.base_log2, ++c, m_col += n) {
            const bool last_col = c + 1 == cols;
            if constexpr (NR > 1) {
                if (c) __syncthreads();              // the previous column's last LDS reads before this column's first LDS writes
            }
            ring_forward_tile_from<A, LT, false, 0, false>(
                v, w, lds,
                [&](int k) {
                    const uint32_t reg = reg_offset<LO0, R0>(k);
                    // (not a streaming load: the same words come back for the next digit)
                    return gadget_digit(gadget_shifted(buf_load64(rx, lane_bytes(reg, x_step), operand_bytes(reg, x_step)), p.q, g), shift, p.q, g);
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
                // every kRingDotF64Period MATRIX columns, as the plain kernel: digits are canonical residues like any other operand
                if ((c & (kRingDotF64Period - 1u)) == kRingDotF64Period - 1u || last_col) {
#pragma unroll
                    for (int r = 0; r < RB; ++r) {
#pragma unroll
                        for (int k = 0; k < kRegs; ++k) acc[r][k] = recentre_f64(acc[r][k], p.qd, p.inv_qd);
                    }
                }
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
