// Ring-element linear combination of device-resident commitment rows (lsr_lwe_ring_combine_rows_device):
//     out_j = sum_{i < terms} p'_{j,i}(X) * row[j * term_stride + i]      component by component in Z_q[X]/(X^n + 1),
// p'_{j,i} = the polynomial whose coefficients are the centred representatives of polys[j][i][x] mod t.  The scalar combine of
// lsr_commit_combine.hpp is the case of constant polynomials.
//
//   ring_combine_prologue_kernel   one workgroup per output: header screening of its term rows (combine_prologue_kernel's), the exact
//                                  integer weight sum_i sum_x |p'_{j,i,x}| against the host-computed budget, status = 1 / 0 / -1, and
//                                  the output row's header
//   ring_combine_lift_kernel       p' as canonical residues under one prime (c' >= 0: c', else q - |c'|) into the workspace; the
//                                  context's forward transform then runs over the workspace in place, once per (output, term, prime),
//                                  and leaves p-hat where the tile kernel reads it
//   ring_combine_tile              n <= 4096.  ntt_tile_ring_dot<A, LT, false, BHAT = true> (lsr_ntt_kernels.hpp) with the first operand
//                                  read straight from the term rows and the result stored straight into the output row: a workgroup owns
//                                  4096 words of the chunk's [outputs][k + 1][n] component space under one prime (RNS: a launch per prime).  Per term:
//                                  the forward rounds of the tile, the product with p-hat at the last-round positions, added into a
//                                  register accumulator with §5c's re-centring period; after the last term the inverse rounds run from
//                                  the accumulator.  A body word >= its modulus lowers the status of its output to -1 in the load.
//   ring_combine_unpack_kernel,    n > 4096 (composed form): the k + 1 components of one output's term rows under one prime as
//   ring_combine_add_kernel        [k + 1][terms][n] for the ring-dot passes (same screening); the sum of two partial results when
//                                  the terms of an output are taken in groups
// Exactness: every operand of the tile kernel is a canonical residue (row words are screened, p' is lifted to a
// canonical residue), so the kernel meets the contracts of ntt_tile_ring_dot term for term: F64 — a product is |r| <= 0.875 q, the
// accumulator is re-centred every kRingDotF64Period products, |acc| < 29 q < 2^50; U64 — canonical products, one conditional
// subtraction per addition.
#pragma once

#include "lsr_arith.hpp"
#include "lsr_commit_combine.hpp"
#include "lsr_ntt_kernels.hpp"

namespace lsr {

struct RingCombineJob {
    const uint64_t* rows;        // [(outputs - 1) * term_stride + terms][row_words], device, only read
    const uint64_t* polys;       // [outputs][terms][n] raw 64-bit words, device
    uint64_t* out;               // [outputs][row_words]
    int* status;                 // [outputs]
    uint64_t terms, term_stride, outputs;
    uint64_t row_words;
    uint32_t header_words;       // 5, RNS: 6
    uint32_t logn;
    uint64_t header[kRnsHeaderWords];   // the header of a row of this context
    uint64_t max_weight;         // combine_max_weight: the largest weight the host comparison of lwe_linear_combine accepts
    PlainScale plain;            // t, 1/t for mod_plain
};

// |c'| of a raw word: c mod t, centred; *negative = the residue lies in (t/2, t)
__device__ __forceinline__ double ring_combine_centred(uint64_t word, const PlainScale& plain, bool* negative) {
    const double cf = mod_plain(word, plain);                      // exact, in [0, t)
    *negative = cf > plain.half;                                   // half = floor(t/2), as combine_centred
    return *negative ? plain.t - cf : cf;
}

// grid = outputs.  status[j] = -1 (a term row with a header that is not this context's) / 0 (over the budget) / 1, header of out[j].
__global__ void __launch_bounds__(256) ring_combine_prologue_kernel(RingCombineJob job) {
    __shared__ unsigned long long weight_sum;
    __shared__ unsigned int any_bad;
    const uint64_t j = blockIdx.x;
    if (threadIdx.x == 0) { weight_sum = 0; any_bad = 0; }
    __syncthreads();
    unsigned long long weight = 0;
    bool bad = false;
    for (uint64_t i = threadIdx.x; i < job.terms; i += 256) {
        const uint64_t* const row = job.rows + (j * job.term_stride + i) * job.row_words;
        for (uint32_t w = 0; w < job.header_words; ++w) bad |= row[w] != job.header[w];
    }
    const uint64_t words = job.terms << job.logn;                   // <= 2^16 2^17
    const uint64_t* const poly = job.polys + j * words;
    for (uint64_t x = threadIdx.x; x < words; x += 256) {
        bool negative;
        weight += (unsigned long long)ring_combine_centred(poly[x], job.plain, &negative);     // < 2^19 each: the sum stays below 2^52
    }
    for (int off = 32; off; off >>= 1) weight += __shfl_xor(weight, off);
    const bool wave_bad = __any(bad);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&weight_sum, weight);
        if (wave_bad) atomicOr(&any_bad, 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) job.status[j] = any_bad ? -1 : (weight_sum <= job.max_weight ? 1 : 0);
    if (threadIdx.x < job.header_words) job.out[j * job.row_words + threadIdx.x] = job.header[threadIdx.x];
}

// dst[o][i][x] = the canonical residue of p'_{o,i,x} under q, for `outputs` outputs x `group` terms; src = the first word of output 0's
// first term of the group, consecutive outputs `src_stride` words apart.  Grid-stride over outputs * group * n words.
__global__ void __launch_bounds__(256) ring_combine_lift_kernel(uint64_t* __restrict__ dst, const uint64_t* __restrict__ src, uint64_t src_stride,
                                                                uint64_t outputs, uint64_t group_words, uint64_t q, PlainScale plain) {
    const uint64_t total = outputs * group_words;
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < total; w += (uint64_t)gridDim.x * 256) {
        const uint64_t o = w / group_words, x = w - o * group_words;
        bool negative;
        const uint64_t mag = (uint64_t)ring_combine_centred(src[o * src_stride + x], plain, &negative);
        dst[w] = negative ? q - mag : mag;                           // mag >= 1 when negative
    }
}

template <class A>
struct RingCombinePrime {
    ModParams p;
    const typename A::twid* fwd;
    const typename A::twid* inv;
    RoundConsts<A> cs;
    const uint64_t* phat;        // [chunk outputs][nterms][n]: the transforms of the lifted polynomials under this prime
    uint64_t block_off;          // words from the start of a row to this prime's residue block
};

struct RingCombineTile {
    const uint64_t* rows;        // term 0 of this launch's group, of the chunk's first output
    uint64_t* out;               // the chunk's first output row
    int* status;                 // the chunk's first status
    uint64_t stride_words;       // term_stride * row_words
    uint64_t row_words;
    uint32_t kp1;                // k + 1 components
    uint32_t nterms;             // terms of this launch
    uint32_t polys;              // chunk outputs * (k + 1)
    uint32_t flags;              // kRingDotFirst / kRingDotLast, as ntt_tile_ring_dot
};

// grid = ceil(polys n / 4096), one launch per prime (selecting the prime's constants inside the kernel costs the registers of both
// sets).  Tile index idx of workgroup b is word idx & (n - 1) of component-space polynomial
// G = (b 4096 + idx) >> LT = output G / (k + 1), component G % (k + 1).
template <class A, int LT>
__global__ void __launch_bounds__(kThreads) ring_combine_tile(RingCombineTile job, RingCombinePrime<A> pr) {
    __shared__ uint64_t lds[kLdsWords];
    constexpr uint32_t NP = kTile >> LT;                                             // polynomials of a tile
    __shared__ uint32_t poly_output[NP];                                             // their outputs; ~0 = past the end (ragged last tile)
    using elem = typename A::elem;
    using twid = typename A::twid;
    constexpr int NR = TileRound<LT, 0>::kCount;
    constexpr int LO0 = TileRound<LT, 0>::LO, R0 = TileRound<LT, 0>::R;               // the mapping the rows are read and written in
    constexpr int LOL = TileRound<LT, NR - 1>::LO, RL = TileRound<LT, NR - 1>::R;    // the shared last-forward / first-inverse mapping
    constexpr uint32_t kMask = (1u << LT) - 1u;
    constexpr uint32_t kAbsent = 0xFFFFFFFFu;
    const ModParams& p = pr.p;
    const uint32_t t = threadIdx.x;
    const uint32_t first_poly = blockIdx.x * NP;
    const uint32_t nmask = kMask;
    const uint32_t block_pos = 0;                                                    // a tile starts at a polynomial's first word
    constexpr bool kOne = LT == kTileLog;                                            // one polynomial per tile: every address is uniform
    if constexpr (!kOne) {
        for (uint32_t pl = t; pl < NP; pl += kThreads) {
            const uint32_t g = first_poly + pl;
            poly_output[pl] = g < job.polys ? g / job.kp1 : kAbsent;
        }
        __syncthreads();
    }
    // kOne: the tile's output and the first word of its component within a row; rows, p-hat and the output go through buffer
    // resources (SGPR base, one lane offset, immediate register offsets), as in ntt_tile_ring_dot
    const uint32_t one_output = kOne ? first_poly / job.kp1 : 0u;
    const uint64_t one_within = pr.block_off + ((uint64_t)(first_poly - one_output * job.kp1) << LT);
    const rsrc_t one_out = make_rsrc(job.out + (uint64_t)one_output * job.row_words + one_within, kTile * 8u);
    const rsrc_t ftab = make_rsrc(pr.fwd, (uint32_t)sizeof(twid) << LT);
    const rsrc_t itab = make_rsrc(pr.inv, (uint32_t)sizeof(twid) << LT);
    const uint32_t lbase = lane_base<LOL, RL>(t);
    const uint32_t base0 = lane_base<LO0, R0>(t);

    // tile index -> chunk output (false: the tile has no such polynomial) and the word's offset within a row of that output
    auto locate = [&](uint32_t idx, uint32_t* jj, uint64_t* within) -> bool {
        const uint32_t pl = idx >> LT;
        const uint32_t o = poly_output[pl];
        if (o == kAbsent) return false;
        const uint32_t comp = first_poly + pl - o * job.kp1;
        *jj = o;
        *within = pr.block_off + ((uint64_t)comp << LT) + (idx & kMask);
        return true;
    };
    bool bad = false;                                                                // kOne: a residue >= q was met
    // word k of round 0 from term row `term` (+ output stride); a residue >= q marks the output
    auto operand_word = [&](const uint64_t* term, int k) -> uint64_t {
        if constexpr (kOne) {
            const rsrc_t r = make_rsrc(term + (uint64_t)one_output * job.stride_words + one_within, kTile * 8u);
            const uint64_t raw = buf_load64<kAuxStream>(r, base0 * 8u, reg_offset<LO0, R0>(k) * 8u);
            bad |= raw >= p.q;
            return raw;
        }
        uint32_t jj;
        uint64_t within;
        if (!locate(base0 | reg_offset<LO0, R0>(k), &jj, &within)) return 0;
        const uint64_t raw = term[(uint64_t)jj * job.stride_words + within];
        if (raw >= p.q) atomicMin(&job.status[jj], -1);
        return raw;
    };
    auto inverse_first = [&](twid (&slot)[kRoundTwiddles]) {
        load_round_twiddles<A, LOL, RL, true, NR == 1>(slot, lbase, block_pos, nmask, p.logn, itab);
    };

    elem v[kRegs], acc[kRegs];
    twid w[2][kRoundTwiddles];
    constexpr int S1 = NR & 1;              // twiddle slot of the first inverse round
#pragma unroll
    for (int k = 0; k < kRegs; ++k) {
        acc[k] = elem_from_bits<A>(0);
        if (!(job.flags & kRingDotFirst)) {
            if constexpr (kOne) {
                acc[k] = elem_from_bits<A>(buf_load64(one_out, lbase * 8u, reg_offset<LOL, RL>(k) * 8u));
                continue;
            }
            uint32_t jj;
            uint64_t within;
            if (locate(lbase | reg_offset<LOL, RL>(k), &jj, &within)) acc[k] = elem_from_bits<A>(job.out[(uint64_t)jj * job.row_words + within]);
        }
    }

    const uint64_t* term = job.rows;
    for (uint32_t i = 0; i < job.nterms; ++i, term += job.row_words) {
        const bool last_term = i + 1 == job.nterms;
        if constexpr (NR > 1) {
            if (i) __syncthreads();                  // the previous term's last LDS reads before this term's first LDS writes
        }
        ring_forward_tile_from<A, LT, false, 0, false>(v, w, lds, [&](int k) { return operand_word(term, k); }, ftab, block_pos, nmask, p,
                                                       [&](twid (&slot)[kRoundTwiddles]) {
                                                           if (last_term) inverse_first(slot);
                                                       });
        if constexpr (kOne) {
            const rsrc_t rb = make_rsrc(pr.phat + (((uint64_t)one_output * job.nterms + i) << LT), kTile * 8u);
#pragma unroll
            for (int k = 0; k < kRegs; ++k) {
                const elem bh = A::load(buf_load64(rb, lbase * 8u, reg_offset<LOL, RL>(k) * 8u), p);
                acc[k] = ring_accumulate<A>(acc[k], ring_product<A>(v[k], bh, p), p);
            }
        } else {
#pragma unroll
        for (int k = 0; k < kRegs; ++k) {
            const uint32_t idx = lbase | reg_offset<LOL, RL>(k);
            const uint32_t o = poly_output[idx >> LT];
            if (o == kAbsent) continue;
            const elem bh = A::load(pr.phat[(((uint64_t)o * job.nterms + i) << LT) + (idx & kMask)], p);
            acc[k] = ring_accumulate<A>(acc[k], ring_product<A>(v[k], bh, p), p);
        }
        }
        if constexpr (std::is_same_v<A, ArithF64>) {
            if ((i & (kRingDotF64Period - 1u)) == kRingDotF64Period - 1u || last_term) {
#pragma unroll
                for (int k = 0; k < kRegs; ++k) acc[k] = recentre_f64(acc[k], p.qd, p.inv_qd);
            }
        }
    }

    if constexpr (kOne) {
        if (bad) atomicMin(&job.status[one_output], -1);
    }
    if (!(job.flags & kRingDotLast)) {               // the re-centred raw accumulator waits in the output row for the next group
#pragma unroll
        for (int k = 0; k < kRegs; ++k) {
            if constexpr (kOne) {
                buf_store64(one_out, lbase * 8u, reg_offset<LOL, RL>(k) * 8u, elem_bits<A>(acc[k]));
                continue;
            }
            uint32_t jj;
            uint64_t within;
            if (locate(lbase | reg_offset<LOL, RL>(k), &jj, &within)) job.out[(uint64_t)jj * job.row_words + within] = elem_bits<A>(acc[k]);
        }
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
        inverse_round<A, LO, R, kLast>(v, w[(S1 + I) & 1], p, pr.cs);
        if constexpr (kLast) {
#pragma unroll
            for (int k = 0; k < kRegs; ++k) {
                if constexpr (kOne) {
                    buf_store64<kAuxStream>(one_out, base * 8u, reg_offset<LO, R>(k) * 8u, A::store_reduced(v[k], p));
                    continue;
                }
                uint32_t jj;
                uint64_t within;
                if (locate(base | reg_offset<LO, R>(k), &jj, &within)) job.out[(uint64_t)jj * job.row_words + within] = A::store_reduced(v[k], p);
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
}

// n > 4096, one output, one prime: dst[c][i][x] = row i's component c (rows = the output's first term row of the group, block = words
// from a row's start to the prime's block); a residue >= q lowers *status to -1.  Grid-stride over kp1 * group * n words.
__global__ void __launch_bounds__(256) ring_combine_unpack_kernel(uint64_t* __restrict__ dst, const uint64_t* __restrict__ rows, uint64_t row_words,
                                                                  uint64_t block, uint32_t kp1, uint64_t group, uint32_t logn, uint64_t q, int* status) {
    const uint64_t total = ((uint64_t)kp1 * group) << logn, nmask = (1ull << logn) - 1;
    bool bad = false;
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < total; w += (uint64_t)gridDim.x * 256) {
        const uint64_t poly = w >> logn, c = poly / group, i = poly - c * group;
        const uint64_t raw = rows[i * row_words + block + (c << logn) + (w & nmask)];
        bad |= raw >= q;
        dst[w] = raw;
    }
    if (bad) atomicMin(status, -1);
}

// acc[x] = acc[x] + part[x] mod q over canonical residues
__global__ void __launch_bounds__(256) ring_combine_add_kernel(uint64_t* __restrict__ acc, const uint64_t* __restrict__ part, uint64_t words, uint64_t q) {
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (uint64_t)gridDim.x * 256) {
        const uint64_t s = acc[w] + part[w];                          // < 2^63
        acc[w] = s >= q ? s - q : s;
    }
}

}  // namespace lsr
