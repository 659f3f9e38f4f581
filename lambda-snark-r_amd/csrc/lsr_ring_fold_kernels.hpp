// Fold of ring VECTORS by ring-valued challenges in the tile (lsr_ring_fold.hip):
//   out[j][c] = sum_{i < terms} p[j][i] * v[j term_stride + i][c],   c < width.
// ntt_tile_ring_dot<A, LT, MID, BHAT = true> (lsr_ntt_kernels.hpp) with one stride generalised and a grid axis over the outputs: the
// transform of challenge p[j][i] is shared by all `width` components of a vector, so it is computed once (launch_ntt into the
// workspace) and read at the last-round positions, as the shared b-hat of the ring inner product.
//
// Operand addressing.  grid.y = output j of the chunk; grid.x tiles the [width][n] words of ONE output.  The components of a vector
// are contiguous, in `out` and in every term vector, so a tile is one run of up to 4096 words whatever n is: at n < 4096 it holds 4096 / n
// consecutive components, and a ragged last tile (width n no multiple of 4096) is clipped by the range of the buffer resources (loads
// read 0, stores are dropped).  The per-output bases are workgroup-uniform 64-bit offsets; term i + 1 of an output lies `a_term`
// (= width n) words behind term i, b-hat_{i+1} n words behind b-hat_i.  Every per-term resource starts at a 64-bit pointer and spans
// one tile, so no operand range approaches 2^31 bytes.
// Accumulator contract: ntt_tile_ring_dot's (one canonical operand b-hat, forward-round outputs |x| < 16 q, |product| <= 0.875 q,
// re-centred every kRingDotF64Period products and after the last: |acc| <= q/2 + 1 + 32 * 0.875 q < 2^50).
#pragma once
#include "lsr_ntt_kernels.hpp"

namespace lsr {

// c: [outputs][total] words (total = width n, a multiple of n).  a: term i of output j at a + j a_out + i a_term, `total` contiguous
// words.  bhat: [outputs][nterms][n], canonical transforms in the order launch_ntt writes.  MID: a holds raw elements left by the
// strided forward rounds, c receives raw elements for the strided inverse round.  flags: kRingDotFirst / kRingDotLast, as
// ntt_tile_ring_dot — a launch sequence over groups of terms keeps its tiling, so every workgroup reads back what it wrote itself.
template <class A, int LT, bool MID>
__global__ void __launch_bounds__(kThreads) ntt_tile_ring_fold(uint64_t* c, const uint64_t* __restrict__ a, const uint64_t* __restrict__ bhat, size_t total,
                                                                 uint32_t nterms, size_t a_term, size_t a_out, uint32_t flags, ModParams p,
                                                                 const typename A::twid* __restrict__ fwd, const typename A::twid* __restrict__ inv,
                                                                 RoundConsts<A> cs) {
    __shared__ uint64_t lds[kLdsWords];
    using elem = typename A::elem;
    using twid = typename A::twid;
    constexpr int NR = TileRound<LT, 0>::kCount;
    constexpr int LO0 = TileRound<LT, 0>::LO, R0 = TileRound<LT, 0>::R;               // the mapping the operands are read in
    constexpr int LOL = TileRound<LT, NR - 1>::LO, RL = TileRound<LT, NR - 1>::R;    // the shared last-forward / first-inverse mapping
    constexpr bool kSeveral = !MID && LT < kTileLog;                                 // several components per tile
    constexpr uint32_t kMask = kSeveral ? (1u << LT) - 1u : 0xFFFFFFFFu;
    const uint32_t t = threadIdx.x;
    const size_t j = blockIdx.y;
    const size_t tile_base = (size_t)blockIdx.x * kTile;
    const uint32_t n = 1u << p.logn;
    const uint32_t nmask = n - 1u;
    const uint32_t block_pos = (uint32_t)(tile_base & nmask);
    const size_t left = total - tile_base;
    const uint32_t tile_bytes = (left >= kTile ? kTile : (uint32_t)left) * 8u;
    const rsrc_t out = make_rsrc(c + j * total + tile_base, tile_bytes);
    const rsrc_t ftab = make_rsrc(fwd, (uint32_t)sizeof(twid) << p.logn);
    const rsrc_t itab = make_rsrc(inv, (uint32_t)sizeof(twid) << p.logn);
    const uint32_t lbase = lane_base<LOL, RL>(t);
    const uint32_t base0 = lane_base<LO0, R0>(t);
    // first inverse round's twiddles; SKIP_TOP when that round is also the transform's last stage
    auto inverse_first = [&](twid (&slot)[kRoundTwiddles]) {
        load_round_twiddles<A, LOL, RL, true, (NR == 1) && !MID>(slot, lbase, block_pos, nmask, p.logn, itab);
    };
    const uint64_t* a_tile = a + j * a_out + tile_base;
    const uint64_t* b_tile = bhat + j * ((size_t)nterms << p.logn);
    const uint32_t b_lane = (MID ? block_pos + lbase : (lbase & kMask)) * 8u;

    elem v[kRegs], acc[kRegs];
    twid w[2][kRoundTwiddles];
    constexpr int S1 = NR & 1;              // twiddle slot of the first inverse round: (S + NR) & 1 of the last forward transform
    if (flags & kRingDotFirst) {
#pragma unroll
        for (int k = 0; k < kRegs; ++k) acc[k] = elem_from_bits<A>(0);
    } else {
#pragma unroll
        for (int k = 0; k < kRegs; ++k) acc[k] = elem_from_bits<A>(buf_load64(out, lbase * 8u, reg_offset<LOL, RL>(k) * 8u));
    }

    for (uint32_t i = 0; i < nterms; ++i, a_tile += a_term, b_tile += n) {
        const bool last_term = i + 1 == nterms;
        if constexpr (NR > 1) {
            if (i) __syncthreads();                  // the previous term's last LDS reads before this term's first LDS writes
        }
        const rsrc_t ra = make_rsrc(a_tile, tile_bytes);
        ring_forward_tile_from<A, LT, MID, 0, false>(
            v, w, lds, [&](int k) { return buf_load64<MID ? 0 : kAuxStream>(ra, base0 * 8u, reg_offset<LO0, R0>(k) * 8u); }, ftab, block_pos, nmask, p,
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

    if (!(flags & kRingDotLast)) {
#pragma unroll
        for (int k = 0; k < kRegs; ++k) buf_store64(out, lbase * 8u, reg_offset<LOL, RL>(k) * 8u, elem_bits<A>(acc[k]));
        return;
    }
#pragma unroll
    for (int k = 0; k < kRegs; ++k) v[k] = acc[k];

    // inverse rounds (ntt_tile_ring_dot's schedule), the first one straight from registers
    static_for<0, NR>([&](auto ic) {
        constexpr int I = decltype(ic)::value;
        constexpr int J = NR - 1 - I;
        constexpr int LO = TileRound<LT, J>::LO, R = TileRound<LT, J>::R;
        constexpr bool kLast = (I == NR - 1);
        constexpr bool kFinal = kLast && !MID;
        const uint32_t base = lane_base<LO, R>(t);
        uint64_t* const row = lds + lds_slot(base);
        if constexpr (I > 0) {
#pragma unroll
            for (int k = 0; k < kRegs; ++k) v[k] = elem_from_bits<A>(row[lds_slot(reg_offset<LO, R>(k))]);
        }
        if constexpr (!kLast) {
            constexpr int LO1 = TileRound<LT, J - 1>::LO, R1 = TileRound<LT, J - 1>::R;
            load_round_twiddles<A, LO1, R1, true, (I + 1 == NR - 1) && !MID>(w[(S1 + I + 1) & 1], lane_base<LO1, R1>(t), block_pos, nmask, p.logn, itab);
        }
        inverse_round<A, LO, R, kFinal>(v, w[(S1 + I) & 1], p, cs);
        if constexpr (!kFinal) {
            constexpr bool kAll = kLast || !A::kPartialRecentre;
#pragma unroll
            for (int k = 0; k < kRegs; ++k)
                if (kAll || A::template needs_recentre<R>(k & ((1 << R) - 1))) A::end_of_inverse_round(v[k], p);
        }
        if constexpr (kLast) {
#pragma unroll
            for (int k = 0; k < kRegs; ++k)
                buf_store64<MID ? 0 : kAuxStream>(out, base * 8u, reg_offset<LO, R>(k) * 8u, MID ? elem_bits<A>(v[k]) : A::store_reduced(v[k], p));
        } else {
            // (I = 0: these are the slots this lane read in the last forward round — no barrier needed before the store)
#pragma unroll
            for (int k = 0; k < kRegs; ++k) row[lds_slot(reg_offset<LO, R>(k))] = elem_bits<A>(v[k]);
            __syncthreads();
        }
    });
}

}  // namespace lsr
