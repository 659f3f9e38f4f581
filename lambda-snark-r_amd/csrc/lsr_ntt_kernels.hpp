// Batched negacyclic NTT kernels for gfx950 (replaces SEAL's ntt_negacyclic_harvey /
// inverse_ntt_negacyclic_harvey behind cpp-core/src/ntt.cpp:84,99).
//
// Decomposition.  A length-n = 2^L transform is L butterfly stages; stage s pairs coefficients whose
// index differs in bit (L-1-s) and multiplies by twiddle[2^s + (index >> (L-s))].  Stages are grouped
// into radix-16 ROUNDS of four consecutive index bits that one lane holds in 16 registers:
//   * tile kernel   — one 256-lane workgroup owns 4096 contiguous residues (one n=4096 polynomial, or
//     4096/n smaller ones, or one 4096-block of a larger one) and runs every round on index bits
//     [0,12) with the tile staged in LDS between rounds (one pad word per 16 keeps the b64 accesses of
//     the radix-16 rounds off each other's banks; PMC: 9 % residual conflict cycles); global traffic is
//     fully coalesced on both ends and goes through buffer resources (SGPR base, one lane offset,
//     immediate register offsets, hardware clipping of a partial last tile).  The 15 twiddles a lane
//     needs for round r+1 are requested before the butterflies of round r start, so their L2 latency
//     hides behind 256 FP64 instructions.
//   * strided round kernel — the top 4 (n = 2^17: 5) index bits of n > 4096: 16 registers hold residues
//     n/16 apart, all 256 lanes of a workgroup walk consecutive addresses, no LDS, twiddles are the
//     first 15 table entries (scalar loads).
//   * inner strided round kernel — n > 2^17 (Goldilocks contexts, up to 2^22): the 4 or 5 index bits between the top round's and the
//     tile's; the upper index bits select its twiddles, the same for all lanes of a workgroup (scalar loads again).
// The intermediate array between two kernels of one transform is private, so it is left in the
// arithmetic's raw element form (f64 bit patterns for ArithF64) — no conversion at pass boundaries.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>

#include "lsr_arith.hpp"
#include "lsr_sampler.hpp"

namespace lsr {

constexpr int kTileLog = 12;
constexpr uint32_t kTile = 1u << kTileLog;
constexpr int kThreads = 256;
constexpr int kRegs = 16;
constexpr int kRoundTwiddles = 15;
constexpr uint32_t kLdsWords = kTile + (kTile >> 4);   // one pad word per 16

template <class A>
struct RoundConsts {
    typename A::twid n_inv;          // n^-1
    typename A::twid w_last_scaled;  // inverse twiddle of the last GS stage times n^-1
};

// padded LDS slot of tile index idx.  For idx = lane part | constant part with disjoint bits the slot splits into
// lds_slot(lane) + lds_slot(constant), so every access is one lane address plus an immediate offset.
__host__ __device__ constexpr uint32_t lds_slot(uint32_t idx) { return idx + (idx >> 4); }

// ---- 6-byte hand-off of the two-pass FP64 transform (PACKED; conversion and bounds: lsr_arith.hpp pack48_from_f64) ----------------
// The private intermediate between the strided round and the tile pass, in place in the caller's array: the 64 consecutive residues
// a wavefront touches in one register row own their 512 bytes — [0, 256) the 64 low dwords, [256, 384) the 64 high halfwords,
// [384, 512) never touched — so every access is whole 128-byte lines and a quarter of the hand-off's bytes stays off the fabric.
// Residue i lives at dword (i & ~63) * 8 + (i & 63) * 4 and halfword (i & ~63) * 8 + 256 + (i & 63) * 2: every index bit has a fixed
// weight, so for i = lane part | register part over disjoint bits both offsets split into one lane offset plus a constant.
// In place without a barrier: the strided rounds read and write a cell from the same wavefront (lane -> consecutive index, 2^lo a
// multiple of 64), and a wavefront's loads have all returned before its first store because every output of the round depends on every
// input; the tile passes own whole cells and put a workgroup barrier between their global loads and stores anyway.
constexpr uint32_t kPackedHalfwords = 256;     // byte offset of a cell's halfwords
template <class T> __host__ __device__ constexpr T packed_lo_bytes(T i) { return ((i & ~(T)63) << 3) + ((i & (T)63) << 2); }
template <class T> __host__ __device__ constexpr T packed_hi_bytes(T i) { return ((i & ~(T)63) << 3) + ((i & (T)63) << 1); }   // + kPackedHalfwords

template <class A> __device__ __forceinline__ uint64_t elem_bits(typename A::elem v);
template <> __device__ __forceinline__ uint64_t elem_bits<ArithF64>(double v) { return (uint64_t)__double_as_longlong(v); }
template <> __device__ __forceinline__ uint64_t elem_bits<ArithU64>(uint64_t v) { return v; }
template <> __device__ __forceinline__ uint64_t elem_bits<ArithGold>(uint64_t v) { return v; }
template <class A> __device__ __forceinline__ typename A::elem elem_from_bits(uint64_t b);
template <> __device__ __forceinline__ double elem_from_bits<ArithF64>(uint64_t b) { return __longlong_as_double((long long)b); }
template <> __device__ __forceinline__ uint64_t elem_from_bits<ArithU64>(uint64_t b) { return b; }
template <> __device__ __forceinline__ uint64_t elem_from_bits<ArithGold>(uint64_t b) { return b; }

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// Round schedule of the tile kernel for LT transformed bits: full radix-16 rounds from the top bit down,
// then one remainder round of LT%4 bits at the bottom.  The inverse runs the same rounds in reverse.
template <int LT, int I>
struct TileRound {
    static constexpr int kFull = LT / 4;
    static constexpr int kRem = LT % 4;
    static constexpr int kCount = kFull + (kRem ? 1 : 0);
    static constexpr int R = I < kFull ? 4 : kRem;
    static constexpr int LO = I < kFull ? LT - 4 * (I + 1) : 0;
};

// Tile index of register k for lane t in a round that keeps bits [LO, LO+R) in registers.  With R < 4
// a lane carries 2^(4-R) independent groups; their selector goes to the top tile bits [8+R, 12).
template <int LO, int R>
__device__ __forceinline__ uint32_t lane_base(uint32_t t) {
    return (t & ((1u << LO) - 1u)) | ((t >> LO) << (LO + R));
}
template <int LO, int R>
__host__ __device__ constexpr uint32_t reg_offset(int k) {
    return (uint32_t)((k & ((1 << R) - 1)) << LO) | (uint32_t)((k >> R) << (8 + R));
}

// ---- twiddles of one round into registers -------------------------------------------------------------
// Order: group, then stage in execution order (forward: high bit first; inverse: low bit first), then u.
// SKIP_TOP: the stage of bit LO+R-1 takes its multipliers from RoundConsts (last inverse stage).
template <class A, int LO, int R, bool INVERSE, bool SKIP_TOP>
__device__ __forceinline__ void load_round_twiddles(typename A::twid (&w)[kRoundTwiddles], uint32_t base_idx, uint32_t block_pos,
                                                    uint32_t nmask, int logn, rsrc_t tw) {
    constexpr int G = 1 << (4 - R);
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const uint32_t pos0 = (block_pos + (base_idx | ((uint32_t)g << (8 + R)))) & nmask;
        static_for<0, R>([&](auto sc) {
            constexpr int step = decltype(sc)::value;
            constexpr int b = INVERSE ? LO + step : LO + R - 1 - step;
            if constexpr (!(SKIP_TOP && b == LO + R - 1)) {
                constexpr int count = 1 << (LO + R - 1 - b);
                // slots before this run: earlier groups, then earlier stages of this group
                constexpr int per_group = (1 << R) - 1 - (SKIP_TOP ? 1 : 0);
                constexpr int before = INVERSE ? ((1 << R) - (1 << (R - step))) : ((1 << step) - 1) - (SKIP_TOP && step > 0 ? 1 : 0);
                const uint32_t tw_base = (1u << (logn - 1 - b)) + (pos0 >> (b + 1));
                A::template load_tw_run<count>(tw, tw_base, &w[g * per_group + before]);
            }
        });
    }
}

// The same slots for the round on tile bits [8, 12) of a 4096-residue block of a larger polynomial (the first forward / last inverse
// round of the LT = 12 pass of a two-pass transform): every stage bit lies above the lane's 8 index bits, so the 15 multipliers depend on
// the block's position alone — workgroup-uniform addresses, plain reads that become scalar loads (SGPR operands, no vector-memory
// instruction, no VGPRs), as in the strided rounds.  profiles/r12_inverse_tile_ablation.txt: the vector twiddle loads own the
// inverse tile pass's whole surplus over the fabric rate.
template <class A, int LO, int R, bool INVERSE>
__device__ __forceinline__ void load_round_twiddles_uniform(typename A::twid (&w)[kRoundTwiddles], uint32_t block_pos, int logn,
                                                            const typename A::twid* __restrict__ tw) {
    static_assert(LO == 8 && R == 4, "the lane index fills bits [0, 8): lane_base<8, 4>(t) = t");
    static_for<0, R>([&](auto sc) {
        constexpr int step = decltype(sc)::value;
        constexpr int b = INVERSE ? LO + step : LO + R - 1 - step;
        constexpr int count = 1 << (LO + R - 1 - b);
        constexpr int before = INVERSE ? ((1 << R) - (1 << (R - step))) : ((1 << step) - 1);
        const uint32_t tw_base = (1u << (logn - 1 - b)) + (block_pos >> (b + 1));     // block_pos is a multiple of 4096
#pragma unroll
        for (int u = 0; u < count; ++u) w[before + u] = A::load_tw(tw, tw_base + u);
    });
}

// ---- butterflies of one round, forward (Cooley–Tukey, high bit first) -----------------------------
// TOP: the round holds the transform's first stages (group index 0 above it).  Flavours with A::kUnitTopTwiddles (cyclic tables:
// entry m + 0 of every stage is omega^0 = 1, lsr_host_math.cpp build_cyclic_twiddles) then skip the product of the u = 0 butterflies —
// 15 of the 32 butterflies of a radix-16 top round, 15.6 % of a 4096-point transform's products.
template <class A, int LO, int R, bool TOP = false>
__device__ __forceinline__ void forward_round(typename A::elem (&v)[kRegs], const typename A::twid (&w)[kRoundTwiddles], const ModParams& p) {
    constexpr int G = 1 << (4 - R);
    int slot = 0;
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int j = R - 1; j >= 0; --j) {          // register bit j <-> index bit LO + j
            const int half = 1 << j;
#pragma unroll
            for (int u = 0; u < (1 << (R - 1 - j)); ++u) {
                const typename A::twid tw = w[slot++];
#pragma unroll
                for (int l = 0; l < half; ++l) {
                    const int kx = (g << R) | (u << (j + 1)) | l;
                    if constexpr (TOP && A::kUnitTopTwiddles) {
                        if (u == 0) A::ct_unit(v[kx], v[kx + half], p);
                        else A::ct(v[kx], v[kx + half], tw, p);
                    } else {
                        A::ct(v[kx], v[kx + half], tw, p);
                    }
                }
            }
        }
    }
}

// ---- butterflies of one round, inverse (Gentleman–Sande, low bit first) ---------------------------
// FINAL: bit LO+R-1 is the transform's last stage (n^-1 folded in, SEAL transform_from_rev's scalar path)
template <class A, int LO, int R, bool FINAL>
__device__ __forceinline__ void inverse_round(typename A::elem (&v)[kRegs], const typename A::twid (&w)[kRoundTwiddles], const ModParams& p,
                                              const RoundConsts<A>& cs) {
    constexpr int G = 1 << (4 - R);
    int slot = 0;
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const int half = 1 << j;
            if (FINAL && j == R - 1) {
#pragma unroll
                for (int l = 0; l < half; ++l) A::gs_scaled(v[(g << R) | l], v[((g << R) | l) + half], cs.w_last_scaled, cs.n_inv, p);
                continue;
            }
#pragma unroll
            for (int u = 0; u < (1 << (R - 1 - j)); ++u) {
                const typename A::twid tw = w[slot++];
#pragma unroll
                for (int l = 0; l < half; ++l) {
                    const int kx = (g << R) | (u << (j + 1)) | l;
                    if constexpr (FINAL && A::kUnitTopTwiddles) {      // the last round = the forward transform's top round: u = 0 is omega^0
                        if (u == 0) A::gs_unit(v[kx], v[kx + half], p);
                        else A::gs(v[kx], v[kx + half], tw, p);
                    } else {
                        A::gs(v[kx], v[kx + half], tw, p);
                    }
                }
            }
        }
    }
}

// ---- tile kernel -----------------------------------------------------------------------------------
// LT = number of low index bits this kernel transforms (min(L,12)).  RAW_IN / RAW_OUT: the global array
// holds raw element bit patterns (pass boundary of a two-pass transform) instead of canonical uint64.
// Global and twiddle accesses go through buffer resources: the tile's base sits in SGPRs, each lane carries
// one byte offset per mapping, register offsets are immediates, and a partial last tile is clipped by the
// resource's size (loads return 0, stores are dropped).
// src (optional): read the operands from there instead of `data` (same layout) — an out-of-place first pass.
// vblock: the tile this workgroup transforms (the hardware block index when the pass is a kernel of its own)
// Elementwise work fused into the read-in of a forward tile pass (the prover's quotient pipeline, lsr_prover.hip; Goldilocks only):
//   MODE 1: every operand is first multiplied by the word of `x1` at the same index (standard form) — the coset product a b;
//   MODE 2: the operands are the c_k of R1CS constraints and x1 = a, x2 = b: a_k b_k == c_k is tested on the way in, a failing
//           constraint marks its instance in `bad` (is_satisfied, r1cs.rs:148-172).  The transform itself is unchanged.
//   MODE 3: MODE 1 on the way in, and on the way OUT the finish of the quotient pipeline (lsr_prover.hip step 6): the transform's
//           output z never reaches memory; Q[j] = (2m)^-1 c_hat[p] - psi^-j (2m)^-1 z[p], p = bitrev(j), is formed where the last round
//           leaves z in registers (c_hat and the untwist table read at the same indices), scattered to its natural-order slot of the
//           LDS tile and streamed out coalesced, with the per-instance highest non-zero index (one atomicMax per wavefront).
struct FuseIn {
    const uint64_t* x1 = nullptr;
    const uint64_t* x2 = nullptr;
    uint32_t* bad = nullptr;
    // MODE 3
    const uint64_t* chat = nullptr;       // [instances][m], same tiling as the data
    const uint64_t* untwist = nullptr;    // [m], Montgomery form
    uint64_t half_m_inv = 0;              // (2m)^-1, Montgomery form
    uint64_t* quotient = nullptr;         // [instances][m], natural order
    uint32_t* top = nullptr;              // [instances]: 1 + highest non-zero index
};
// PACKED (RAW_IN, FP64): the raw operands arrive in the 6-byte hand-off layout above.
template <class A, int LT, bool RAW_IN, bool RAW_OUT, int MODE = 0, bool PACKED = false>
__device__ __forceinline__ void tile_forward_body(uint64_t* __restrict__ data, size_t total, const ModParams& p,
                                                  const typename A::twid* __restrict__ tw, const uint64_t* __restrict__ src, uint32_t vblock,
                                                  const FuseIn& fuse = FuseIn{}) {
    static_assert(!PACKED || (RAW_IN && !RAW_OUT && MODE == 0 && std::is_same_v<A, ArithF64>), "6-byte hand-off: second pass of the FP64 forward transform");
    __shared__ uint64_t lds[kLdsWords];
    using elem = typename A::elem;
    using twid = typename A::twid;
    constexpr int NR = TileRound<LT, 0>::kCount;
    const uint32_t t = threadIdx.x;
    const size_t tile_base = (size_t)vblock * kTile;
    const uint32_t nmask = (1u << p.logn) - 1u;
    const uint32_t block_pos = (uint32_t)(tile_base & nmask);
    const size_t left = total - tile_base;
    const uint32_t tile_bytes = left >= kTile ? kTile * 8u : (uint32_t)left * 8u;
    const rsrc_t tile = make_rsrc(data + tile_base, tile_bytes);
    const rsrc_t from = make_rsrc(const_cast<uint64_t*>(src ? src : data) + tile_base, tile_bytes);
    const rsrc_t table = make_rsrc(tw, (uint32_t)sizeof(twid) << p.logn);
    elem v[kRegs];
    twid w[2][kRoundTwiddles];

    {   // first round: operands straight from global memory in the round's own mapping
        constexpr int LO = TileRound<LT, 0>::LO, R = TileRound<LT, 0>::R;
        const uint32_t base = lane_base<LO, R>(t);
        uint64_t raw[PACKED ? 1 : kRegs];
        uint32_t low[PACKED ? kRegs : 1];
        int16_t high[PACKED ? kRegs : 1];
        if constexpr (PACKED) {
            const uint32_t lane_lo = packed_lo_bytes(base), lane_hi = packed_hi_bytes(base);
#pragma unroll
            for (int k = 0; k < kRegs; ++k) {
                low[k] = buf_load32<kAuxStream>(from, lane_lo, packed_lo_bytes(reg_offset<LO, R>(k)));
                high[k] = buf_load16s<kAuxStream>(from, lane_hi, packed_hi_bytes(reg_offset<LO, R>(k)) + kPackedHalfwords);
            }
        } else {
#pragma unroll
            for (int k = 0; k < kRegs; ++k) raw[k] = buf_load64<RAW_OUT ? 0 : kAuxStream>(from, base * 8u, reg_offset<LO, R>(k) * 8u);
        }
        if constexpr (A::kScalarTopTwiddles && LT == kTileLog && RAW_IN) load_round_twiddles_uniform<A, LO, R, false>(w[0], block_pos, p.logn, tw);
        else load_round_twiddles<A, LO, R, false, false>(w[0], base, block_pos, nmask, p.logn, table);
        if constexpr (PACKED) {
#pragma unroll
            for (int k = 0; k < kRegs; ++k) v[k] = f64_from_pack48(low[k], high[k]);
        } else if constexpr (MODE == 0) {
#pragma unroll
            for (int k = 0; k < kRegs; ++k) v[k] = RAW_IN ? elem_from_bits<A>(raw[k]) : A::load(raw[k], p);
        } else {
            static_assert(std::is_same_v<A, ArithGold> && !RAW_IN, "fused elementwise work: first pass of a Goldilocks transform");
            const rsrc_t r1 = make_rsrc(fuse.x1 + tile_base, tile_bytes);
            if constexpr (MODE == 1 || MODE == 3) {
                uint64_t o1[kRegs];
#pragma unroll
                for (int k = 0; k < kRegs; ++k) o1[k] = buf_load64(r1, base * 8u, reg_offset<LO, R>(k) * 8u);
#pragma unroll
                for (int k = 0; k < kRegs; ++k) v[k] = gold_mul(A::load(raw[k], p), A::load(o1[k], p));
            } else {
                // a and b come in two halves: three operand sets live at once cost 138 VGPRs and a wave of occupancy
                const rsrc_t r2 = make_rsrc(fuse.x2 + tile_base, tile_bytes);
#pragma unroll
                for (int k = 0; k < kRegs; ++k) v[k] = A::load(raw[k], p);
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    constexpr int H = kRegs / 2;
                    uint64_t o1[H], o2[H];
#pragma unroll
                    for (int k = 0; k < H; ++k) {
                        o1[k] = buf_load64(r1, base * 8u, reg_offset<LO, R>(half * H + k) * 8u);
                        o2[k] = buf_load64(r2, base * 8u, reg_offset<LO, R>(half * H + k) * 8u);
                    }
#pragma unroll
                    for (int k = 0; k < H; ++k) {
                        const uint32_t at = base + reg_offset<LO, R>(half * H + k);     // index within the tile
                        if (at * 8u < tile_bytes && gold_mul(A::load(o1[k], p), A::load(o2[k], p)) != v[half * H + k])
                            atomicOr(&fuse.bad[(tile_base + at) >> p.logn], 1u);         // only ever taken for an unsatisfied instance
                    }
                }
            }
        }
    }

    static_for<0, NR>([&](auto ic) {
        constexpr int I = decltype(ic)::value;
        constexpr int LO = TileRound<LT, I>::LO, R = TileRound<LT, I>::R;
        const uint32_t base = lane_base<LO, R>(t);
        if constexpr (I + 1 < NR) {   // request the next round's twiddles before this round's arithmetic
            constexpr int LO1 = TileRound<LT, I + 1>::LO, R1 = TileRound<LT, I + 1>::R;
            load_round_twiddles<A, LO1, R1, false, false>(w[(I + 1) & 1], lane_base<LO1, R1>(t), block_pos, nmask, p.logn, table);
        }
        forward_round<A, LO, R, I == 0 && !RAW_IN && (LO + R == LT)>(v, w[I & 1], p);   // !RAW_IN: this pass is the whole transform (LT = log n)
        uint64_t* const row = lds + lds_slot(base);
#pragma unroll
        for (int k = 0; k < kRegs; ++k) row[lds_slot(reg_offset<LO, R>(k))] = elem_bits<A>(v[k]);
        __syncthreads();
        if constexpr (I + 1 < NR) {
            constexpr int LO1 = TileRound<LT, I + 1>::LO, R1 = TileRound<LT, I + 1>::R;
            const uint64_t* const row1 = lds + lds_slot(lane_base<LO1, R1>(t));
#pragma unroll
            for (int k = 0; k < kRegs; ++k) v[k] = elem_from_bits<A>(row1[lds_slot(reg_offset<LO1, R1>(k))]);
        }
    });

    // coalesced write-out: lane t stores tile indices t + 256 k
    const uint64_t* const col = lds + lds_slot(t);
    if constexpr (MODE == 3) {
        // The finish, in the coalesced mapping (the last round's own mapping holds 16 consecutive words per lane: c_hat and the
        // untwist table would be read with a 128-byte lane stride, measured 100 us per 2^24 words).  Lane t takes z at tile indices
        // p = t + 256 k (bit-reversed order), forms Q there, and a second trip through the tile puts Q at its natural index.
        // Slot map of that trip: nat + (nat >> S), S = log m - 6 — a wavefront's 64 natural indices are 2^S apart (bit reversal
        // of consecutive p), the pad spreads them over all banks; the coalesced read-back stays conflict-free.
        constexpr int S = LT >= 10 ? LT - 6 : 4;
        const rsrc_t chat = make_rsrc(fuse.chat + tile_base, tile_bytes);
        const rsrc_t untw = make_rsrc(fuse.untwist, 8u << p.logn);
        const rsrc_t out = make_rsrc(fuse.quotient + tile_base, tile_bytes);
        uint64_t h[kRegs];
        {
            uint64_t c[kRegs], uw[kRegs];
#pragma unroll
            for (int k = 0; k < kRegs; ++k) {
                c[k] = buf_load64<kAuxStream>(chat, t * 8u, (uint32_t)k * kThreads * 8u);
                uw[k] = buf_load64(untw, ((block_pos + t + (uint32_t)k * kThreads) & nmask) * 8u, 0);
            }
#pragma unroll
            for (int k = 0; k < kRegs; ++k)   // z is a lazy 64-bit representative (ArithGold::ct): gold_mul_mont takes any
                h[k] = gold_sub(gold_mul_mont(A::load(c[k], p), fuse.half_m_inv), gold_mul_mont(col[lds_slot((uint32_t)k * kThreads)], uw[k]));
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kRegs; ++k) {
            const uint32_t at = t + (uint32_t)k * kThreads;
            const uint32_t nat = (at & ~nmask) | (__brev(at & nmask) >> (32 - LT));       // LT = log m (single-pass transform)
            lds[nat + (nat >> S)] = h[k];
        }
        __syncthreads();
        constexpr int kGroup = LT >= 8 ? 1 << (LT - 8) : 1;     // registers per instance
#pragma unroll
        for (int g = 0; g < kRegs / kGroup; ++g) {
            uint32_t best = 0;                                   // wave-uniform for log m >= 6
#pragma unroll
            for (int kk = 0; kk < kGroup; ++kk) {
                const int k = g * kGroup + kk;
                const uint32_t at = t + (uint32_t)k * kThreads;
                const bool live = at * 8u < tile_bytes;
                const uint64_t q = lds[at + (at >> S)];
                buf_store64<kAuxStream>(out, t * 8u, (uint32_t)k * kThreads * 8u, q);
                if constexpr (LT >= 6) {   // a wavefront's 64 consecutive words belong to one instance: one atomic per wavefront and instance
                    const uint64_t nz = __ballot(live && q != 0);
                    if (nz) best = ((at & ~63u) & nmask) + 64u - (uint32_t)__clzll(nz);
                } else if (live && q != 0) {
                    atomicMax(&fuse.top[(tile_base + at) >> p.logn], (at & nmask) + 1u);
                }
            }
            if constexpr (LT >= 6) {
                const uint32_t first = t + (uint32_t)(g * kGroup) * kThreads;
                if (best && (t & 63u) == 0) atomicMax(&fuse.top[(tile_base + first) >> p.logn], best);
            }
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < kRegs; ++k) {
        const uint64_t bits = col[lds_slot((uint32_t)k * kThreads)];
        buf_store64<RAW_OUT ? 0 : kAuxStream>(tile, t * 8u, (uint32_t)k * kThreads * 8u, RAW_OUT ? bits : A::store_canonical(elem_from_bits<A>(bits), p));
    }
}
template <class A, int LT, bool RAW_IN, bool RAW_OUT, bool PACKED = false>
__global__ void __launch_bounds__(kThreads) ntt_tile_forward(uint64_t* __restrict__ data, size_t total, ModParams p,
                                                               const typename A::twid* __restrict__ tw, const uint64_t* __restrict__ src = nullptr) {
    tile_forward_body<A, LT, RAW_IN, RAW_OUT, 0, PACKED>(data, total, p, tw, src, blockIdx.x);
}
template <class A, int LT, int MODE>
__global__ void __launch_bounds__(kThreads) ntt_tile_forward_fused(uint64_t* __restrict__ data, size_t total, ModParams p,
                                                                     const typename A::twid* __restrict__ tw, const uint64_t* __restrict__ src, FuseIn fuse) {
    tile_forward_body<A, LT, false, false, MODE>(data, total, p, tw, src, blockIdx.x, fuse);
}

// `add` (optional, only when !RAW_OUT): canonical residues added to the outputs on the final store — the fused
// discrete-Gaussian blinding add of the commitment (u = INTT(...) + e1).
// PRE: every input word is first multiplied by pre[its index within the polynomial] (canonical residues) — a diagonal
// operator fused into the read-in (the coset twist of the prover's quotient pipeline, lsr_prover.hip).
// DEFER (first pass of a two-pass inverse, flavours with A::kDeferredRecentre): the last round's outputs are stored as they leave the
// butterflies, |x| <= 32 q; the strided round that follows re-centres them on load (strided_round_body RECENTRE_IN), where the VALU idles.
// PACKED (RAW_OUT, FP64, never with DEFER: the un-centred words need 50 bits): the last round re-centres its outputs, |x| <= q / 2 + 1,
// and stores them in the 6-byte hand-off layout.
template <class A, int LT, bool RAW_IN, bool RAW_OUT, bool PRE = false, bool DEFER = false, bool PACKED = false>
__device__ __forceinline__ void tile_inverse_body(uint64_t* __restrict__ data, size_t total, const ModParams& p,
                                                  const typename A::twid* __restrict__ tw, const RoundConsts<A>& cs,
                                                  const uint64_t* __restrict__ add, const uint64_t* __restrict__ pre, uint32_t vblock) {
    static_assert(!DEFER || (RAW_OUT && A::kDeferredRecentre), "deferred re-centring: the raw hand-off of a flavour that re-centres");
    static_assert(!PACKED || (RAW_OUT && !RAW_IN && !DEFER && std::is_same_v<A, ArithF64>), "6-byte hand-off: first pass of the FP64 inverse transform, re-centred");
    __shared__ uint64_t lds[kLdsWords];
    using elem = typename A::elem;
    using twid = typename A::twid;
    constexpr int NR = TileRound<LT, 0>::kCount;
    const uint32_t t = threadIdx.x;
    const size_t tile_base = (size_t)vblock * kTile;
    const uint32_t nmask = (1u << p.logn) - 1u;
    const uint32_t block_pos = (uint32_t)(tile_base & nmask);
    const size_t left = total - tile_base;
    const uint32_t tile_bytes = left >= kTile ? kTile * 8u : (uint32_t)left * 8u;
    const rsrc_t tile = make_rsrc(data + tile_base, tile_bytes);
    const rsrc_t table = make_rsrc(tw, (uint32_t)sizeof(twid) << p.logn);
    elem v[kRegs];
    twid w[2][kRoundTwiddles];

    {   // coalesced read-in to LDS (raw element bits); the first round's twiddles ride along
        uint64_t raw[kRegs];
        // single-pass inverse transforms (n <= 4096): a fresh workgroup puts its loads in flight ahead of its neighbours' arithmetic
        // (-4 % at n = 4096; the same in the forward kernel or in the passes of a two-pass transform loses 2-3 %: profiles/r02b_tile_prio.txt)
        constexpr bool kLoadPrio = !RAW_IN && !RAW_OUT;
        if constexpr (kLoadPrio) __builtin_amdgcn_s_setprio(3);
#pragma unroll
        for (int k = 0; k < kRegs; ++k) raw[k] = buf_load64<RAW_OUT ? 0 : kAuxStream>(tile, t * 8u, (uint32_t)k * kThreads * 8u);
        if constexpr (kLoadPrio) __builtin_amdgcn_s_setprio(0);
        constexpr int J = NR - 1;
        constexpr int LO = TileRound<LT, J>::LO, R = TileRound<LT, J>::R;
        load_round_twiddles<A, LO, R, true, (NR == 1) && !RAW_OUT>(w[0], lane_base<LO, R>(t), block_pos, nmask, p.logn, table);
        uint64_t* const col = lds + lds_slot(t);
        if constexpr (PRE) {
            static_assert(!RAW_IN, "the fused diagonal multiply belongs to the first pass");
            const rsrc_t diag = make_rsrc(pre, 8u << p.logn);
            uint64_t d[kRegs];
#pragma unroll
            for (int k = 0; k < kRegs; ++k) d[k] = buf_load64(diag, ((block_pos + t + (uint32_t)k * kThreads) & nmask) * 8u, 0);
#pragma unroll
            for (int k = 0; k < kRegs; ++k) col[lds_slot((uint32_t)k * kThreads)] = elem_bits<A>(A::pre_mul(A::load(raw[k], p), d[k], p));
        } else {
#pragma unroll
            for (int k = 0; k < kRegs; ++k) col[lds_slot((uint32_t)k * kThreads)] = RAW_IN ? raw[k] : elem_bits<A>(A::load(raw[k], p));
        }
    }
    __syncthreads();

    static_for<0, NR>([&](auto ic) {
        constexpr int I = decltype(ic)::value;          // I-th inverse round = forward round NR-1-I
        constexpr int J = NR - 1 - I;
        constexpr int LO = TileRound<LT, J>::LO, R = TileRound<LT, J>::R;
        constexpr bool kLast = (I == NR - 1);
        constexpr bool kFinal = kLast && !RAW_OUT;      // outputs of the n^-1-scaled stage (LT == log n)
        const uint32_t base = lane_base<LO, R>(t);
        uint64_t* const row = lds + lds_slot(base);
#pragma unroll
        for (int k = 0; k < kRegs; ++k) v[k] = elem_from_bits<A>(row[lds_slot(reg_offset<LO, R>(k))]);
        if constexpr (!kLast) {
            constexpr int J1 = J - 1;
            constexpr int LO1 = TileRound<LT, J1>::LO, R1 = TileRound<LT, J1>::R;
            constexpr bool kNextFinal = (I + 1 == NR - 1) && !RAW_OUT;
            if constexpr (A::kScalarTopTwiddles && LT == kTileLog && RAW_OUT && J1 == 0) load_round_twiddles_uniform<A, LO1, R1, true>(w[(I + 1) & 1], block_pos, p.logn, tw);
            else load_round_twiddles<A, LO1, R1, true, kNextFinal>(w[(I + 1) & 1], lane_base<LO1, R1>(t), block_pos, nmask, p.logn, table);
        }
        uint64_t blind[(kLast && !RAW_OUT) ? kRegs : 1];
        if constexpr (kLast && !RAW_OUT) {   // request the blinding residues before the last round's arithmetic
            if (add != nullptr) {
                const rsrc_t extra = make_rsrc(add + tile_base, tile_bytes);
#pragma unroll
                for (int k = 0; k < kRegs; ++k) blind[k] = buf_load64(extra, base * 8u, reg_offset<LO, R>(k) * 8u);
            }
        }
        inverse_round<A, LO, R, kFinal>(v, w[I & 1], p, cs);
        if constexpr (!kFinal && !(DEFER && kLast)) {
            // inner rounds re-centre only the outputs that can exceed the next round's 2 q input bound (lsr_arith.hpp needs_recentre);
            // the last round of a first pass (RAW_OUT) re-centres everything: the strided round that follows runs up to five stages
            // (DEFER: that round does it on load)
            constexpr bool kAll = kLast || !A::kPartialRecentre;
#pragma unroll
            for (int k = 0; k < kRegs; ++k)
                if (kAll || A::template needs_recentre<R>(k & ((1 << R) - 1))) A::end_of_inverse_round(v[k], p);
        }
        if constexpr (kLast) {
            if (!RAW_OUT && add != nullptr) {
#pragma unroll
                for (int k = 0; k < kRegs; ++k)
                    buf_store64<kAuxStream>(tile, base * 8u, reg_offset<LO, R>(k) * 8u, A::store_reduced_plus(v[k], blind[k], p));
            } else if constexpr (PACKED) {
                const uint32_t lane_lo = packed_lo_bytes(base), lane_hi = packed_hi_bytes(base);
#pragma unroll
                for (int k = 0; k < kRegs; ++k) {
                    uint32_t low;
                    uint16_t high;
                    pack48_from_f64(v[k], low, high);
                    buf_store32(tile, lane_lo, packed_lo_bytes(reg_offset<LO, R>(k)), low);
                    buf_store16(tile, lane_hi, packed_hi_bytes(reg_offset<LO, R>(k)) + kPackedHalfwords, high);
                }
            } else {
#pragma unroll
                for (int k = 0; k < kRegs; ++k)
                    buf_store64<RAW_OUT ? 0 : kAuxStream>(tile, base * 8u, reg_offset<LO, R>(k) * 8u, RAW_OUT ? elem_bits<A>(v[k]) : A::store_reduced(v[k], p));
            }
        } else {
#pragma unroll
            for (int k = 0; k < kRegs; ++k) row[lds_slot(reg_offset<LO, R>(k))] = elem_bits<A>(v[k]);
            __syncthreads();
        }
    });
}
template <class A, int LT, bool RAW_IN, bool RAW_OUT, bool PRE = false, bool DEFER = false, bool PACKED = false>
__global__ void __launch_bounds__(kThreads) ntt_tile_inverse(uint64_t* __restrict__ data, size_t total, ModParams p,
                                                               const typename A::twid* __restrict__ tw, RoundConsts<A> cs,
                                                               const uint64_t* __restrict__ add, const uint64_t* __restrict__ pre = nullptr) {
    tile_inverse_body<A, LT, RAW_IN, RAW_OUT, PRE, DEFER, PACKED>(data, total, p, tw, cs, add, pre, blockIdx.x);
}

// ---- ring multiply c = a b in the tile (lsr_ring_mul.hip) --------------------------------------------
// One workgroup: forward rounds of its tile of a, forward rounds of the same tile of b, the product in registers, inverse rounds,
// store.  The last forward round and the first inverse round share the mapping TileRound<LT, NR-1>, so a-hat (16 registers) and
// b-hat meet in registers and the product feeds the inverse without an LDS round trip.
// MID: the middle pass of an n > 4096 product — a and b hold raw elements left by the strided forward rounds, c receives raw
// elements for the strided inverse round (c may be a: in place).  BHAT: b is the transform of ONE polynomial ([n] words, canonical,
// the order launch_ntt writes), read at the last-round positions instead of transformed.
// Product at the boundary (flavour-specific): inputs are forward-round outputs, the result must meet the inverse
// rounds' input contract (F64: |x| <= 2 q; U64: [0, 2q); Gold: canonical).
template <class A> __device__ __forceinline__ typename A::elem ring_product(typename A::elem x, typename A::elem y, const ModParams& p);
template <> __device__ __forceinline__ double ring_product<ArithF64>(double x, double y, const ModParams& p) {
    // |x|, |y| < 16 q (17 CT stages, each adding < 0.875 q); one canonical operand and |x| < 2^50 make the product exact, |r| <= 0.875 q
    return mulmod_f64(x, canonical_f64(y, p.qd, p.inv_qd), p.qd, p.inv_qd);
}
template <> __device__ __forceinline__ uint64_t ring_product<ArithU64>(uint64_t x, uint64_t y, const ModParams& p) {
    return mulmod_barrett128(x, y, p);   // lazy [0, 4q) operands: the Barrett product takes any 64-bit pair, canonical out
}
template <> __device__ __forceinline__ uint64_t ring_product<ArithGold>(uint64_t x, uint64_t y, const ModParams&) {
    return gold_mul(x, y);               // lazy 64-bit representatives: the 128-bit reduction takes any pair, canonical out
}

// Forward rounds of one tile operand, left in v at the last round's mapping (no LDS store after the last round).  Round I uses the
// twiddle slot w[(S + I) & 1]; PRELOADED: round 0's twiddles are already in w[S].  `after` fills w[(S + NR) & 1] while the last round
// computes (the next phase's first twiddles).
template <class A, int LT, bool RAW, int S, bool PRELOADED, class After>
__device__ __forceinline__ void ring_forward_tile(typename A::elem (&v)[kRegs], typename A::twid (&w)[2][kRoundTwiddles], uint64_t* lds, rsrc_t from,
                                                  rsrc_t table, uint32_t block_pos, uint32_t nmask, const ModParams& p, After&& after) {
    constexpr int NR = TileRound<LT, 0>::kCount;
    const uint32_t t = threadIdx.x;
    {
        constexpr int LO = TileRound<LT, 0>::LO, R = TileRound<LT, 0>::R;
        const uint32_t base = lane_base<LO, R>(t);
        uint64_t raw[kRegs];
#pragma unroll
        for (int k = 0; k < kRegs; ++k) raw[k] = buf_load64<RAW ? 0 : kAuxStream>(from, base * 8u, reg_offset<LO, R>(k) * 8u);
        if constexpr (!PRELOADED) load_round_twiddles<A, LO, R, false, false>(w[S & 1], base, block_pos, nmask, p.logn, table);
#pragma unroll
        for (int k = 0; k < kRegs; ++k) v[k] = RAW ? elem_from_bits<A>(raw[k]) : A::load(raw[k], p);
    }
    static_for<0, NR>([&](auto ic) {
        constexpr int I = decltype(ic)::value;
        constexpr int LO = TileRound<LT, I>::LO, R = TileRound<LT, I>::R;
        if constexpr (I + 1 < NR) {
            constexpr int LO1 = TileRound<LT, I + 1>::LO, R1 = TileRound<LT, I + 1>::R;
            load_round_twiddles<A, LO1, R1, false, false>(w[(S + I + 1) & 1], lane_base<LO1, R1>(t), block_pos, nmask, p.logn, table);
        } else {
            after(w[(S + NR) & 1]);
        }
        forward_round<A, LO, R, I == 0 && !RAW && (LO + R == LT)>(v, w[(S + I) & 1], p);
        if constexpr (I + 1 < NR) {
            uint64_t* const row = lds + lds_slot(lane_base<LO, R>(t));
#pragma unroll
            for (int k = 0; k < kRegs; ++k) row[lds_slot(reg_offset<LO, R>(k))] = elem_bits<A>(v[k]);
            __syncthreads();
            constexpr int LO1 = TileRound<LT, I + 1>::LO, R1 = TileRound<LT, I + 1>::R;
            const uint64_t* const row1 = lds + lds_slot(lane_base<LO1, R1>(t));
#pragma unroll
            for (int k = 0; k < kRegs; ++k) v[k] = elem_from_bits<A>(row1[lds_slot(reg_offset<LO1, R1>(k))]);
        }
    });
}

template <class A, int LT, bool MID, bool BHAT>
__global__ void __launch_bounds__(kThreads) ntt_tile_ring_mul(uint64_t* c, const uint64_t* a, const uint64_t* b, size_t total, ModParams p,
                                                                const typename A::twid* __restrict__ fwd, const typename A::twid* __restrict__ inv,
                                                                RoundConsts<A> cs) {
    // (no __restrict__ on c, a, b: c may alias either; every load of the tile precedes the first store)
    __shared__ uint64_t lds[kLdsWords];
    using elem = typename A::elem;
    using twid = typename A::twid;
    constexpr int NR = TileRound<LT, 0>::kCount;
    constexpr int LOL = TileRound<LT, NR - 1>::LO, RL = TileRound<LT, NR - 1>::R;    // the shared last-forward / first-inverse mapping
    const uint32_t t = threadIdx.x;
    const size_t tile_base = (size_t)blockIdx.x * kTile;
    const uint32_t nmask = (1u << p.logn) - 1u;
    const uint32_t block_pos = (uint32_t)(tile_base & nmask);
    const size_t left = total - tile_base;
    const uint32_t tile_bytes = left >= kTile ? kTile * 8u : (uint32_t)left * 8u;
    const rsrc_t out = make_rsrc(c + tile_base, tile_bytes);
    const rsrc_t ra = make_rsrc(a + tile_base, tile_bytes);
    const rsrc_t ftab = make_rsrc(fwd, (uint32_t)sizeof(twid) << p.logn);
    const rsrc_t itab = make_rsrc(inv, (uint32_t)sizeof(twid) << p.logn);
    const uint32_t lbase = lane_base<LOL, RL>(t);
    // first inverse round's twiddles; SKIP_TOP when that round is also the transform's last stage
    auto inverse_first = [&](twid (&slot)[kRoundTwiddles]) {
        load_round_twiddles<A, LOL, RL, true, (NR == 1) && !MID>(slot, lbase, block_pos, nmask, p.logn, itab);
    };
    elem v[kRegs];
    twid w[2][kRoundTwiddles];
    constexpr int S1 = BHAT ? NR & 1 : 0;   // twiddle slot of the first inverse round: (S + NR) & 1 of the last forward transform

    if constexpr (BHAT) {
        ring_forward_tile<A, LT, MID, 0, false>(v, w, lds, ra, ftab, block_pos, nmask, p, inverse_first);
        // b-hat at this lane's last-round positions within the polynomial (one polynomial's transform: stays L2-resident)
        const rsrc_t rb = make_rsrc(b, 8u << p.logn);
        constexpr uint32_t kMask = MID ? 0xFFFFFFFFu : (1u << LT) - 1u;          // n <= 4096: the tile holds 4096 / n polynomials
        const uint32_t lane_off = MID ? block_pos + lbase : (lbase & kMask);
#pragma unroll
        for (int k = 0; k < kRegs; ++k) v[k] = ring_product<A>(v[k], A::load(buf_load64(rb, lane_off * 8u, (reg_offset<LOL, RL>(k) & kMask) * 8u), p), p);
    } else {
        elem ah[kRegs];
        // a's last round prefetches b's first-round twiddles (round 0 of the same table) into the free slot
        ring_forward_tile<A, LT, MID, 0, false>(v, w, lds, ra, ftab, block_pos, nmask, p, [&](twid (&slot)[kRoundTwiddles]) {
            constexpr int LO0 = TileRound<LT, 0>::LO, R0 = TileRound<LT, 0>::R;
            load_round_twiddles<A, LO0, R0, false, false>(slot, lane_base<LO0, R0>(t), block_pos, nmask, p.logn, ftab);
        });
#pragma unroll
        for (int k = 0; k < kRegs; ++k) ah[k] = v[k];
        if constexpr (NR > 1) __syncthreads();       // a's last LDS reads before b's first LDS writes
        const rsrc_t rb = make_rsrc(b + tile_base, tile_bytes);
        ring_forward_tile<A, LT, MID, NR & 1, true>(v, w, lds, rb, ftab, block_pos, nmask, p, inverse_first);
#pragma unroll
        for (int k = 0; k < kRegs; ++k) v[k] = ring_product<A>(ah[k], v[k], p);
    }

    // inverse rounds (tile_inverse_body's schedule), the first one straight from registers
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

// ---- ring inner product c = sum_i a_i b_i in the tile (lsr_ring_dot.hip) ------------------------------
// ntt_tile_ring_mul with a loop over the terms around its forward half: per term the forward rounds of the tile of a_i, the
// forward rounds of the tile of b_i (or b-hat_i read at the last-round positions), the product added into a register accumulator
// that sits at the last-forward / first-inverse mapping; after the last term the inverse rounds run from the accumulator.
//
// Operand addressing.  The words of term i that belong to ONE output are n contiguous words; consecutive outputs' term-i polynomials
// are `os` words apart (os = terms n for a [batch][terms][n] operand).  n = 4096 and MID: the tile is one run of 4096 words.  n < 4096
// (kStrided): tile index idx = output (idx >> LT) | coefficient (idx & (n - 1)) lies at (idx & (n - 1)) + (idx >> LT) os.  Every
// mapping writes idx as lane part | register part over disjoint bits, so both terms split into one lane offset plus one
// workgroup-uniform register offset, as in the contiguous kernels.
// Accumulator contract: F64 — a product is |r| <= 0.875 q, the accumulator is re-centred to |acc| <= q/2 + 1 after
// every kRingDotF64Period products and after the last one, so |acc| <= (0.5 + 0.875 * 32) q + 1 < 29 q < 2^50: every sum is an exact
// integer in a double and inside recentre_f64's domain, and the inverse rounds receive |x| <= q/2 + 1 <= 2 q.  U64: canonical
// products, one conditional subtraction per addition (sums stay below 2 q < 2^62).  Goldilocks: gold_add.
constexpr uint32_t kRingDotF64Period = 32;
constexpr uint32_t kRingDotFirst = 1u, kRingDotLast = 2u;
constexpr uint32_t kRingDotOutOfRange = 0x80000000u;   // a lane offset beyond every operand range (ranges stay below 2^31 bytes)

template <class A> __device__ __forceinline__ typename A::elem ring_accumulate(typename A::elem acc, typename A::elem r, const ModParams& p);
template <> __device__ __forceinline__ double ring_accumulate<ArithF64>(double acc, double r, const ModParams&) { return acc + r; }
template <> __device__ __forceinline__ uint64_t ring_accumulate<ArithU64>(uint64_t acc, uint64_t r, const ModParams& p) {
    const uint64_t s = acc + r;
    return s >= p.q ? s - p.q : s;
}
template <> __device__ __forceinline__ uint64_t ring_accumulate<ArithGold>(uint64_t acc, uint64_t r, const ModParams&) { return gold_add(acc, r); }

// ring_forward_tile with the operand words fetched by `load(k)` (the raw word of register k in round 0's mapping) instead of read from
// one contiguous tile.
template <class A, int LT, bool RAW, int S, bool PRELOADED, class Load, class After>
__device__ __forceinline__ void ring_forward_tile_from(typename A::elem (&v)[kRegs], typename A::twid (&w)[2][kRoundTwiddles], uint64_t* lds, Load&& load,
                                                       rsrc_t table, uint32_t block_pos, uint32_t nmask, const ModParams& p, After&& after) {
    constexpr int NR = TileRound<LT, 0>::kCount;
    const uint32_t t = threadIdx.x;
    {
        constexpr int LO = TileRound<LT, 0>::LO, R = TileRound<LT, 0>::R;
        uint64_t raw[kRegs];
#pragma unroll
        for (int k = 0; k < kRegs; ++k) raw[k] = load(k);
        if constexpr (!PRELOADED) load_round_twiddles<A, LO, R, false, false>(w[S & 1], lane_base<LO, R>(t), block_pos, nmask, p.logn, table);
#pragma unroll
        for (int k = 0; k < kRegs; ++k) v[k] = RAW ? elem_from_bits<A>(raw[k]) : A::load(raw[k], p);
    }
    static_for<0, NR>([&](auto ic) {
        constexpr int I = decltype(ic)::value;
        constexpr int LO = TileRound<LT, I>::LO, R = TileRound<LT, I>::R;
        if constexpr (I + 1 < NR) {
            constexpr int LO1 = TileRound<LT, I + 1>::LO, R1 = TileRound<LT, I + 1>::R;
            load_round_twiddles<A, LO1, R1, false, false>(w[(S + I + 1) & 1], lane_base<LO1, R1>(t), block_pos, nmask, p.logn, table);
        } else {
            after(w[(S + NR) & 1]);
        }
        forward_round<A, LO, R, I == 0 && !RAW && (LO + R == LT)>(v, w[(S + I) & 1], p);
        if constexpr (I + 1 < NR) {
            uint64_t* const row = lds + lds_slot(lane_base<LO, R>(t));
#pragma unroll
            for (int k = 0; k < kRegs; ++k) row[lds_slot(reg_offset<LO, R>(k))] = elem_bits<A>(v[k]);
            __syncthreads();
            constexpr int LO1 = TileRound<LT, I + 1>::LO, R1 = TileRound<LT, I + 1>::R;
            const uint64_t* const row1 = lds + lds_slot(lane_base<LO1, R1>(t));
#pragma unroll
            for (int k = 0; k < kRegs; ++k) v[k] = elem_from_bits<A>(row1[lds_slot(reg_offset<LO1, R1>(k))]);
        }
    });
}

// c: [outputs][n], `total` words.  a: term i of output j at a + j a_os + i n; b likewise with b_os — or, BHAT, the transforms of the
// `nterms` polynomials of ONE shared b ([nterms][n], canonical, the order launch_ntt writes).  MID: a and b hold raw elements left
// by the strided forward rounds, c receives raw elements for the strided inverse round.
// flags: kRingDotFirst — the accumulator starts at zero (else: at the raw accumulator an earlier launch left in c);
//        kRingDotLast  — inverse rounds and the final store (else: the re-centred raw accumulator goes to c at the last-round positions
//                        for the launch that takes the next terms).  A launch sequence over groups of terms keeps its tiling, so every
//                        workgroup reads back what it wrote itself.
template <class A, int LT, bool MID, bool BHAT>
__global__ void __launch_bounds__(kThreads) ntt_tile_ring_dot(uint64_t* c, const uint64_t* __restrict__ a, const uint64_t* __restrict__ b, size_t total,
                                                                uint32_t nterms, size_t a_os, size_t b_os, uint32_t flags, ModParams p,
                                                                const typename A::twid* __restrict__ fwd, const typename A::twid* __restrict__ inv,
                                                                RoundConsts<A> cs) {
    __shared__ uint64_t lds[kLdsWords];
    using elem = typename A::elem;
    using twid = typename A::twid;
    constexpr int NR = TileRound<LT, 0>::kCount;
    constexpr int LO0 = TileRound<LT, 0>::LO, R0 = TileRound<LT, 0>::R;               // the mapping the operands are read in
    constexpr int LOL = TileRound<LT, NR - 1>::LO, RL = TileRound<LT, NR - 1>::R;    // the shared last-forward / first-inverse mapping
    constexpr bool kStrided = !MID && LT < kTileLog;                                 // several outputs per tile
    constexpr uint32_t kMask = kStrided ? (1u << LT) - 1u : 0xFFFFFFFFu;
    const uint32_t t = threadIdx.x;
    const size_t tile_base = (size_t)blockIdx.x * kTile;
    const uint32_t n = 1u << p.logn;
    const uint32_t nmask = n - 1u;
    const uint32_t block_pos = (uint32_t)(tile_base & nmask);
    const size_t left = total - tile_base;
    const uint32_t tile_words = left >= kTile ? kTile : (uint32_t)left;
    const size_t first_output = tile_base >> p.logn;
    const uint32_t outputs = kStrided ? tile_words >> LT : 1u;                        // (total is a multiple of n)
    const rsrc_t out = make_rsrc(c + tile_base, tile_words * 8u);
    const rsrc_t ftab = make_rsrc(fwd, (uint32_t)sizeof(twid) << p.logn);
    const rsrc_t itab = make_rsrc(inv, (uint32_t)sizeof(twid) << p.logn);
    const uint32_t lbase = lane_base<LOL, RL>(t);
    const uint32_t base0 = lane_base<LO0, R0>(t);

    // byte offset of tile index part `idx` (a lane part or a register part) in an operand whose outputs are `os` words apart
    auto operand_bytes = [&](uint32_t idx, uint32_t os) -> uint32_t {
        return kStrided ? ((idx & kMask) + (idx >> LT) * os) * 8u : idx * 8u;
    };
    // Word k of round 0 from the operand tile at `tile` (os: as above).  A partial last tile (fewer than 4096 / n outputs) is clipped
    // twice: by the range of the buffer resource, and — the outputs being far apart — by an out-of-range lane offset for every word
    // of an output the tile does not have.
    auto operand_words = [&](uint32_t os) -> uint32_t { return kStrided ? (outputs - 1u) * os + n : tile_words; };
    auto operand_word = [&](rsrc_t r, uint32_t os, int k) -> uint64_t {
        const uint32_t reg = reg_offset<LO0, R0>(k);
        const bool present = !kStrided || (base0 >> LT) + (reg >> LT) < outputs;
        return buf_load64<MID ? 0 : kAuxStream>(r, present ? operand_bytes(base0, os) : kRingDotOutOfRange, operand_bytes(reg, os));
    };
    const uint32_t a_step = (uint32_t)a_os, b_step = (uint32_t)b_os;                  // used when kStrided only: terms n <= 2^27 there
    // first inverse round's twiddles; SKIP_TOP when that round is also the transform's last stage
    auto inverse_first = [&](twid (&slot)[kRoundTwiddles]) {
        load_round_twiddles<A, LOL, RL, true, (NR == 1) && !MID>(slot, lbase, block_pos, nmask, p.logn, itab);
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
            ring_forward_tile_from<A, LT, MID, 0, false>(v, w, lds, [&](int k) { return operand_word(ra, a_step, k); }, ftab, block_pos, nmask, p,
                                                         [&](twid (&slot)[kRoundTwiddles]) {
                                                             if (last_term) inverse_first(slot);
                                                         });
            // b-hat_i at this lane's last-round positions within the polynomial
            const rsrc_t rb = make_rsrc(b_tile, 8u << p.logn);
            const uint32_t lane_off = MID ? block_pos + lbase : (lbase & kMask);
#pragma unroll
            for (int k = 0; k < kRegs; ++k) {
                const elem bh = A::load(buf_load64(rb, lane_off * 8u, (reg_offset<LOL, RL>(k) & kMask) * 8u), p);
                acc[k] = ring_accumulate<A>(acc[k], ring_product<A>(v[k], bh, p), p);
            }
        } else {
            elem ah[kRegs];
            // a's last round prefetches b's first-round twiddles (round 0 of the same table) into the free slot
            ring_forward_tile_from<A, LT, MID, 0, false>(v, w, lds, [&](int k) { return operand_word(ra, a_step, k); }, ftab, block_pos, nmask, p,
                                                         [&](twid (&slot)[kRoundTwiddles]) {
                                                             load_round_twiddles<A, LO0, R0, false, false>(slot, base0, block_pos, nmask, p.logn, ftab);
                                                         });
#pragma unroll
            for (int k = 0; k < kRegs; ++k) ah[k] = v[k];
            if constexpr (NR > 1) __syncthreads();   // a's last LDS reads before b's first LDS writes
            const rsrc_t rb = make_rsrc(b_tile, operand_words(b_step) * 8u);
            ring_forward_tile_from<A, LT, MID, NR & 1, true>(v, w, lds, [&](int k) { return operand_word(rb, b_step, k); }, ftab, block_pos, nmask, p,
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

    // inverse rounds (ntt_tile_ring_mul's schedule), the first one straight from registers
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

// ---- strided round kernel (the TOP R index bits: lo + R == log n) ------------------------------------
// Its butterfly groups are indexed by the polynomial only, so stage j (register bit j) uses the table entries
// 2^(R-1-j) + u for every lane of every polynomial: compile-time indices, scalar loads, no VGPRs for twiddles.
// ADD: canonical residues `add` are added to the outputs in the final store (inverse, last pass only).
// Forward rounds (ADD is then false): a non-null `add` is the array to READ the operands from (out-of-place first pass).
// SM (sampling mode; 1 and 2 with ADD): the blinding residues are not read from `add` but SAMPLED in the passes around the middle
// stage — the CDT Gaussian of lsr_sampler.hpp, object = polynomial (key bs.keys[4 (poly / components)], stream index
// poly % components).  A workgroup owns 256 columns x 2^R rows of one polynomial = 2^R * 32 ChaCha blocks of 8 consecutive
// coefficients; the samples change hands through LDS.  The operand loads are issued first and are in flight under the cipher
// work, so the integer-bound sampler and the memory-bound round share a pass, and e1 never exists in memory as residues.
//   SM = 1: the last inverse round samples all 2^R rows itself (2^R / 8 blocks per lane);
//   SM = 3 + SM = 2: the FORWARD round of the same chunk (its VALU is as idle as the inverse round's) samples rows [0, 2^R / 2) and
//            leaves them in bs.side as int8, one byte per row packed per column ([polynomial][column][2^R / 16] words: 1/16 of a
//            polynomial pass); the inverse round reads that and samples rows [2^R / 2, 2^R) — the cipher work split over two passes.
//            Needs table entries <= 127 (magnitudes fit a byte).
// RECENTRE_IN (last pass of run_ntt's two-pass inverse, whose tile pass ran with DEFER): the raw operands are the un-centred outputs
// of the tile pass's last round, index bits [lo - 4, lo).  1: re-centre the words of the class that can exceed 2 q (needs_recentre:
// index bits lo - 2 and lo - 1 clear — the same for a lane's 2^R words, and for a whole wavefront since lo >= 9); 2: re-centre all.
// PACKED (run_ntt's FP64 two-pass transform when the context allows it): the raw side of the round — the outputs of a forward round, the
// operands of an inverse one — is in the 6-byte hand-off layout (top of this file); the canonical side is unchanged.
template <class A, int R, bool INVERSE, bool RAW_IN, bool RAW_OUT, bool ADD, int SM, int RECENTRE_IN = 0, bool PACKED = false>
__device__ __forceinline__ void strided_round_body(uint64_t* __restrict__ data, size_t total, int lo, ModParams p,
                                                   const typename A::twid* __restrict__ tw, RoundConsts<A> cs,
                                                   const uint64_t* __restrict__ add, const BlindSampler& bs, uint32_t vblock = blockIdx.x,
                                                   uint32_t vthread = threadIdx.x) {
    // vblock / vthread: the 256-lane group this call plays (a kernel that hosts the round as ONE of its roles, lsr_commit_fused.hpp
    // mlwe_mixed, passes its own numbering; sampling modes use the real indices and LDS and are not available there)
    static_assert(!ADD || (INVERSE && !RAW_OUT), "the fused add belongs to the last inverse pass");
    static_assert(SM == 0 || R >= 4, "2^R / 16 blocks per lane and half");
    static_assert((SM != 1 && SM != 2) || ADD, "sampling replaces the read of the blinding residues");
    static_assert(SM != 3 || (!INVERSE && !ADD), "the forward round only prepares samples");
    static_assert(RECENTRE_IN == 0 || (INVERSE && RAW_IN && !RAW_OUT && SM == 0 && A::kDeferredRecentre), "deferred re-centring: run_ntt's last inverse pass");
    static_assert(RECENTRE_IN != 1 || R <= 4, "five stages need every operand re-centred (32 sums of 1.75 q pass 2^50 for q near 2^45)");
    static_assert(!PACKED || (std::is_same_v<A, ArithF64> && SM == 0 && RECENTRE_IN == 0 && RAW_IN == INVERSE && RAW_OUT == !INVERSE),
                  "6-byte hand-off: the two strided rounds of run_ntt<ArithF64>, re-centred operands");
    using elem = typename A::elem;
    constexpr int N = 1 << R;
    const size_t group = (size_t)vblock * kThreads + vthread;
    if (group >= (total >> R)) return;          // whole workgroups: total >> R is a multiple of kThreads (2^lo >= 512)
    const size_t low = group & (((size_t)1 << lo) - 1);
    const size_t idx0 = ((group >> lo) << (lo + R)) | low;
    elem v[N];
    uint64_t extra[ADD ? N : 1];
    const uint64_t* const from = (!INVERSE && add != nullptr) ? add : data;
    // streaming policy: the last pass of an inverse transform, and operands read out of place (the caller's array is read once)
    const bool stream_in = (LSR_NT_LAST_PASS && INVERSE && !RAW_OUT) || (LSR_NT_COMMIT_INPUTS && !INVERSE && add != nullptr);
    // (PACKED: row k of a lane's words starts k << lo residues = (k << lo) * 8 bytes further on — 2^lo is a multiple of the 64-residue cell)
    // In place the same bytes are read as uint64_t and written as uint32_t / uint16_t (forward; the inverse round the other way round),
    // types that type-based alias analysis treats as disjoint, so the compiler is NOT held to program order by the addresses.  What holds
    // it — and, in the hardware, what makes every load of the wavefront return before its first store issues — is data dependence alone:
    // each stored value is a function of all 2^R loaded ones (R full butterfly stages).  A variant of this round whose outputs did not
    // depend on every input (a partial round, a copy-through row) would need an explicit fence between its loads and its stores.
    char* const cell_lo = reinterpret_cast<char*>(data) + packed_lo_bytes(idx0);
    char* const cell_hi = reinterpret_cast<char*>(data) + packed_hi_bytes(idx0) + kPackedHalfwords;
    if constexpr (PACKED && RAW_IN) {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const uint32_t* const pl = reinterpret_cast<const uint32_t*>(cell_lo + ((size_t)k << (lo + 3)));
            const int16_t* const ph = reinterpret_cast<const int16_t*>(cell_hi + ((size_t)k << (lo + 3)));
            const uint32_t low = stream_in ? __builtin_nontemporal_load(pl) : *pl;
            const int16_t high = stream_in ? __builtin_nontemporal_load(ph) : *ph;
            v[k] = f64_from_pack48(low, high);
        }
    } else if (stream_in) {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const uint64_t raw = __builtin_nontemporal_load(from + idx0 + ((size_t)k << lo));
            v[k] = RAW_IN ? elem_from_bits<A>(raw) : A::load(raw, p);
        }
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const uint64_t raw = from[idx0 + ((size_t)k << lo)];
            v[k] = RAW_IN ? elem_from_bits<A>(raw) : A::load(raw, p);
        }
    }
    if constexpr (RECENTRE_IN != 0) {
        if (RECENTRE_IN == 2 || ((low >> (lo - 2)) & 3u) == 0) {
#pragma unroll
            for (int k = 0; k < N; ++k) A::end_of_inverse_round(v[k], p);
        }
    }
    if constexpr (SM != 0) {
        extern __shared__ uint64_t lds_words[];
        uint64_t* const cdf63 = lds_words;
        uint64_t* const tile_words = lds_words + ((bs.entries + 1u) & ~1u);
        const bool in_lanes = lane_table_steps(bs.entries) != 0u;            // the table in the wavefront's lanes (cdt_search), else in LDS
        if (!in_lanes) {
            for (uint32_t i = threadIdx.x; i < bs.entries; i += kThreads) cdf63[i] = bs.cdf[i] >> 1;
            __syncthreads();
        }
        const LaneTable tab = in_lanes ? lane_table_load(bs.cdf, bs.entries) : LaneTable{0u, 0u};
        const size_t g0 = (size_t)blockIdx.x * kThreads;               // workgroup-uniform: polynomial and first column
        const uint32_t poly = (uint32_t)(g0 >> lo), low0 = (uint32_t)(g0 & (((size_t)1 << lo) - 1));
        const uint64_t* const key = bs.keys + 4 * (size_t)(poly / bs.components);
        constexpr int kRows = SM == 1 ? N : N / 2;                      // rows sampled by this pass
        constexpr int kRow0 = SM == 2 ? N / 2 : 0;                      // first of them
        constexpr int kSideWords = N / 16;                              // packed words per column in bs.side
#pragma unroll 1
        for (int h = 0; h < kRows / 8; ++h) {
            const uint32_t b = (uint32_t)h * kThreads + threadIdx.x, row = b >> 5, cb = b & 31u;
            uint64_t w[8], u[8];
            stream_block(key, bs.domain, poly % bs.components, ((((kRow0 + row) << lo) + low0) >> 3) + cb, w);
#pragma unroll
            for (int i = 0; i < 8; ++i) u[i] = w[i] >> 1;
            uint32_t magnitude[8];
            cdt_magnitudes(tab, cdf63, bs.entries, u, magnitude);
            if constexpr (SM == 3) {                                    // int8 tile [row][256 columns]: eight samples = one LDS word
                uint64_t packed = 0;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const uint32_t m = magnitude[i], sign = (uint32_t)(w[i] & 1ull);
                    packed |= (uint64_t)((sign ? 0u - m : m) & 0xFFu) << (8 * i);
                }
                tile_words[row * (kThreads / 8) + cb] = packed;
            } else {                                                    // int32 tile [row][256 columns]
                int32_t* const tile = reinterpret_cast<int32_t*>(tile_words);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int32_t m = (int32_t)magnitude[i], sign = (int32_t)(w[i] & 1ull);
                    tile[row * kThreads + cb * 8 + i] = sign ? -m : m;
                }
            }
        }
        __syncthreads();
        if constexpr (SM == 3) {                                        // column j: one byte per row, packed row-major into words
            const uint8_t* const bytes = reinterpret_cast<const uint8_t*>(tile_words);
            uint64_t* const dst = bs.side + ((size_t)poly << lo) * kSideWords + (size_t)(low0 + threadIdx.x) * kSideWords;
#pragma unroll
            for (int wd = 0; wd < kSideWords; ++wd) {
                uint64_t packed = 0;
#pragma unroll
                for (int i = 0; i < 8; ++i) packed |= (uint64_t)bytes[(wd * 8 + i) * kThreads + threadIdx.x] << (8 * i);
                dst[wd] = packed;
            }
        } else {
            const int32_t* const tile = reinterpret_cast<const int32_t*>(tile_words);
            if constexpr (SM == 2) {
                const uint64_t* const src = bs.side + ((size_t)poly << lo) * kSideWords + (size_t)(low0 + threadIdx.x) * kSideWords;
#pragma unroll
                for (int wd = 0; wd < kSideWords; ++wd) {
                    const uint64_t packed = __builtin_nontemporal_load(src + wd);
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const int32_t e = (int32_t)(int8_t)(packed >> (8 * i));
                        extra[wd * 8 + i] = e < 0 ? p.q - (uint64_t)(-e) : (uint64_t)e;
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < kRows; ++k) {
                const int32_t e = tile[k * kThreads + threadIdx.x];
                extra[kRow0 + k] = e < 0 ? p.q - (uint64_t)(-e) : (uint64_t)e;
            }
        }
    } else if constexpr (ADD) {   // the blinding residues travel with the operands, not behind the arithmetic
#pragma unroll
        for (int k = 0; k < N; ++k) extra[k] = LSR_NT_COMMIT_INPUTS ? __builtin_nontemporal_load(add + idx0 + ((size_t)k << lo)) : add[idx0 + ((size_t)k << lo)];
    }
    if (!INVERSE) {
#pragma unroll
        for (int j = R - 1; j >= 0; --j) {
            const int half = 1 << j;
#pragma unroll
            for (int u = 0; u < (1 << (R - 1 - j)); ++u) {
                const typename A::twid w = tw[(1 << (R - 1 - j)) + u];
#pragma unroll
                for (int l = 0; l < half; ++l) {
                    const int kx = (u << (j + 1)) | l;
                    A::ct(v[kx], v[kx + half], w, p);
                }
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const int half = 1 << j;
            if (!RAW_OUT && j == R - 1) {   // the transform's last stage (bit log n - 1)
#pragma unroll
                for (int l = 0; l < half; ++l) A::gs_scaled(v[l], v[l + half], cs.w_last_scaled, cs.n_inv, p);
                continue;
            }
#pragma unroll
            for (int u = 0; u < (1 << (R - 1 - j)); ++u) {
                const typename A::twid w = tw[(1 << (R - 1 - j)) + u];
#pragma unroll
                for (int l = 0; l < half; ++l) {
                    const int kx = (u << (j + 1)) | l;
                    A::gs(v[kx], v[kx + half], w, p);
                }
            }
        }
        if (RAW_OUT) {
#pragma unroll
            for (int k = 0; k < N; ++k) A::end_of_inverse_round(v[k], p);
        }
    }
    if constexpr (PACKED && RAW_OUT) {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            uint32_t low;
            uint16_t high;
            pack48_from_f64(v[k], low, high);
            *reinterpret_cast<uint32_t*>(cell_lo + ((size_t)k << (lo + 3))) = low;
            *reinterpret_cast<uint16_t*>(cell_hi + ((size_t)k << (lo + 3))) = high;
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const size_t gi = idx0 + ((size_t)k << lo);
        uint64_t out;
        if (RAW_OUT) out = elem_bits<A>(v[k]);
        else if constexpr (ADD) out = A::store_reduced_plus(v[k], extra[k], p);
        else out = INVERSE ? A::store_reduced(v[k], p) : A::store_canonical(v[k], p);
        if constexpr (LSR_NT_LAST_PASS && INVERSE && !RAW_OUT) __builtin_nontemporal_store(out, data + gi);
        else data[gi] = out;
    }
}

template <class A, int R, bool INVERSE, bool RAW_IN, bool RAW_OUT, bool ADD, int RECENTRE_IN = 0, bool PACKED = false>
__global__ void __launch_bounds__(kThreads) ntt_strided_round(uint64_t* __restrict__ data, size_t total, int lo, ModParams p,
                                                                const typename A::twid* __restrict__ tw, RoundConsts<A> cs,
                                                                const uint64_t* __restrict__ add) {
    strided_round_body<A, R, INVERSE, RAW_IN, RAW_OUT, ADD, 0, RECENTRE_IN, PACKED>(data, total, lo, p, tw, cs, add, BlindSampler{});
}

// last pass of an inverse transform with the blinding residues sampled in place (dynamic LDS: table + sample tile); HALF: the first
// half of the rows comes from bs.side, written by ntt_strided_round_sampling of the same chunk
template <class A, int R, bool RAW_IN, bool HALF>
__global__ void __launch_bounds__(kThreads) ntt_strided_round_sampled(uint64_t* __restrict__ data, size_t total, int lo, ModParams p,
                                                                        const typename A::twid* __restrict__ tw, RoundConsts<A> cs, BlindSampler bs) {
    strided_round_body<A, R, true, RAW_IN, false, true, HALF ? 2 : 1>(data, total, lo, p, tw, cs, nullptr, bs);
}
// first (out-of-place, raw-out) round of a forward transform that also samples the first half of the rows of the blinding
// polynomial of the same index into bs.side
template <class A, int R>
__global__ void __launch_bounds__(kThreads) ntt_strided_round_sampling(uint64_t* __restrict__ data, size_t total, int lo, ModParams p,
                                                                         const typename A::twid* __restrict__ tw, RoundConsts<A> cs,
                                                                         const uint64_t* __restrict__ src, BlindSampler bs) {
    strided_round_body<A, R, false, false, true, false, 3>(data, total, lo, p, tw, cs, src, bs);
}

// ---- inner strided round (index bits [lo, lo + R) with lo + R < log n: the second round of an n > 2^17 transform) ----
// Stage s of the transform multiplies by twiddle[2^s + (index >> (L - s))]: for register bit j (index bit lo + j) that is entry
// ((2^H + h) << (R-1-j)) + u, with H = log n - lo - R, h = the index bits above the round and u = the register bits above j.  The top
// round is the case H = 0, h = 0.  A workgroup's 256 lanes walk consecutive addresses and lo >= 8, so h (taken from the block index
// alone) is the same for all of them and the 2^R - 1 twiddles are scalar loads like the top round's (runs of 2^(R-1-j) consecutive
// entries per stage).  Raw elements in and out, in place; the inverse mirrors the forward (Gentleman-Sande, low bit first, inverse
// table).  Exactness: the round runs the butterflies A::ct / A::gs of the other rounds on their own hand-off contract; for
// Goldilocks forward values are any 64-bit representative and inverse values canonical (lsr_arith.hpp), whatever the number of
// rounds.  The F64 / U64 flavours bound their raw values by the number of stages between reductions and are not carried through a
// third pass: lsr_ntt.hip instantiates this kernel for ArithGold only.  (No unit-twiddle skip: only h = 0 has omega^0 entries.)
template <class A, int R, bool INVERSE>
__global__ void __launch_bounds__(kThreads) ntt_inner_round(uint64_t* __restrict__ data, size_t total, int lo, ModParams p,
                                                              const typename A::twid* __restrict__ tw) {
    using elem = typename A::elem;
    constexpr int N = 1 << R;
    const uint32_t per_high = 1u << (lo - 8);                       // workgroups per value of the upper bits
    const size_t high = (size_t)(blockIdx.x >> (lo - 8));          // polynomial | index bits above the round: workgroup-uniform
    const size_t low = (size_t)((blockIdx.x & (per_high - 1u)) << 8) | threadIdx.x;
    const size_t idx0 = (high << (lo + R)) | low;
    if (idx0 + ((size_t)(N - 1) << lo) >= total) return;            // (the grid is exact: total >> R is a multiple of kThreads)
    const int hbits = p.logn - lo - R;
    const uint32_t tbase = (1u << hbits) | ((uint32_t)high & ((1u << hbits) - 1u));
    elem v[N];
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = elem_from_bits<A>(data[idx0 + ((size_t)k << lo)]);
    if (!INVERSE) {
#pragma unroll
        for (int j = R - 1; j >= 0; --j) {
            const int half = 1 << j;
#pragma unroll
            for (int u = 0; u < (1 << (R - 1 - j)); ++u) {
                const typename A::twid w = tw[(tbase << (R - 1 - j)) + u];
#pragma unroll
                for (int l = 0; l < half; ++l) {
                    const int kx = (u << (j + 1)) | l;
                    A::ct(v[kx], v[kx + half], w, p);
                }
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const int half = 1 << j;
#pragma unroll
            for (int u = 0; u < (1 << (R - 1 - j)); ++u) {
                const typename A::twid w = tw[(tbase << (R - 1 - j)) + u];
#pragma unroll
                for (int l = 0; l < half; ++l) {
                    const int kx = (u << (j + 1)) | l;
                    A::gs(v[kx], v[kx + half], w, p);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < N; ++k) A::end_of_inverse_round(v[k], p);
    }
#pragma unroll
    for (int k = 0; k < N; ++k) data[idx0 + ((size_t)k << lo)] = elem_bits<A>(v[k]);
}

// ---- pointwise product (ntt.cpp:106-119) ------------------------------------------------------------
static __global__ void __launch_bounds__(kThreads) pointwise_mul_kernel(uint64_t* __restrict__ out, const uint64_t* __restrict__ a,
                                                                          const uint64_t* __restrict__ b, size_t count, ModParams p) {
    const size_t stride = (size_t)gridDim.x * kThreads;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < count; i += stride) out[i] = mulmod_barrett128(a[i], b[i], p);
}

static __global__ void __launch_bounds__(kThreads) pointwise_mul_gold_kernel(uint64_t* __restrict__ out, const uint64_t* __restrict__ a,
                                                                               const uint64_t* __restrict__ b, size_t count) {
    const size_t stride = (size_t)gridDim.x * kThreads;
    const ModParams unused{};
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < count; i += stride)
        out[i] = gold_mul(ArithGold::load(a[i], unused), ArithGold::load(b[i], unused));
}

// out[b][i] = in[b][bitrev(i)] — boundary permutation between the natural order of rust-api/lambda-snark/src/ntt.rs and the
// bit-reversed order the butterfly network produces/consumes
static __global__ void __launch_bounds__(kThreads) bit_reverse_kernel(uint64_t* __restrict__ out, const uint64_t* __restrict__ in, int logn,
                                                                        size_t total) {
    const size_t stride = (size_t)gridDim.x * kThreads;
    const uint32_t mask = (1u << logn) - 1u;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += stride) {
        const uint32_t lane = (uint32_t)i & mask;
        out[i] = in[(i - lane) + (__brev(lane) >> (32 - logn))];
    }
}

}  // namespace lsr
