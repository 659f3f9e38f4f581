// Two-prime RNS commitments: one commitment under Q = q1 q2 ~ 2^88 held as its residues mod two 44-bit NTT primes,
// so that lwe_linear_combine has the reference's range (any coefficient below t, cpp-core/src/commitment.cpp:88-96,247-266) while
// every transform and product stays on the exact FP64-FMA Barrett kernels (q_i < 2^45, lsr_arith.hpp).
//
//   u_i = INTT_qi(A_i^T NTT_qi(r)) + e1          v_i = INTT_qi(<b_i, NTT_qi(r)>) + e2 + (round(Q (m mod t) / t) mod q_i)
// r, e1, e2 are small integers that do not depend on the modulus: sampled ONCE per commitment and fed to both primes.
// Wire row: data[0] = payload bytes; payload = {"LSRR0001", n | k<<32, q1, q2, t, u_1[k][n], v_1[n], u_2[k][n], v_2[n]}.
//
// "rns-tile" (n = 4096, FP64 flavour, rank <= 4, CDT table <= 64 entries): ONE launch, one 512-lane workgroup per commitment /
// opening — f8_tile_pipeline (lsr_commit_fused.hpp) run once per prime inside the same workgroup; the samples of the first pass stay
// in LDS as int8 (|sample| <= 63 for such a table) for the second.
// "rns-general": the general kernels (lsr_commit_kernels.hpp) once per prime, plus the elementwise kernels below.
#pragma once

#include "lsr_commit_tile.hpp"

namespace lsr {

constexpr uint32_t kRnsHeaderWords = 6;                           // data[0] + 5 header words
constexpr uint64_t kRnsMagic = 0x313030305252534CULL;             // "LSRR0001"

// constants of one RNS context (host-built, passed by value)
struct RnsConsts {
    uint64_t q[2];           // q1, q2
    uint64_t t;              // plaintext modulus
    uint64_t qt;             // Q mod t
    uint64_t tinv[2];        // t^-1 mod q_i
    uint64_t q1inv;          // q1^-1 mod q2
    uint64_t big_lo, big_hi; // Q = q1 q2 < 2^88
    double inv_q1, inv_q2;   // 1 / q_i, for the quotient estimate of the decode
};

__host__ __device__ inline uint64_t rns_header_word(uint32_t w, uint64_t row_words, uint64_t shape, const RnsConsts& rc) {
    return w == 0 ? 8ull * (row_words - 1) : (w == 1 ? kRnsMagic : (w == 2 ? shape : (w == 3 ? rc.q[0] : (w == 4 ? rc.q[1] : rc.t))));
}

// round(Q m' / t) mod q_i for m' < t, without ever forming the 108-bit product: with h = (t - 1) / 2 (t is an odd prime, so the
// rounding has no ties) and rho = (Q m' + h) mod t = ((Q mod t) m' + h) mod t  [< 2^41 before the reduction],
//     round(Q m' / t) = (Q m' + h - rho) / t   exactly, hence   == (h - rho) t^-1   (mod q_i)   because q_i | Q.
// One 64-bit remainder and one Barrett product; h - rho lies in (-t, t).
__device__ __forceinline__ uint64_t rns_message_term(uint64_t word, const RnsConsts& rc, int i, const ModParams& p) {
    const uint64_t mm = word % rc.t, h = rc.t >> 1;
    const uint64_t rho = (rc.qt * mm + h) % rc.t;
    const uint64_t d = h >= rho ? h - rho : p.q - (rho - h);
    return mulmod_barrett128(d, rc.tinv[i], p);
}
// the same in FP64 for the tile sink (the embed sits in the lanes of the transforms): |result| <= 0.875 q_i
struct RnsPlainScale {
    PlainScale ps;           // t, 1/t, -, Q mod t, (t - 1) / 2
    double tinv;             // t^-1 mod q_i
};
__host__ __device__ inline RnsPlainScale make_rns_plain_scale(const RnsConsts& rc, int i) {
    return RnsPlainScale{PlainScale{(double)rc.t, 1.0 / (double)rc.t, 0.0, (double)rc.qt, (double)(rc.t >> 1)}, (double)rc.tinv[i]};
}
__device__ __forceinline__ double rns_embed_plain(uint64_t word, const RnsPlainScale& m, const ModParams& p) {
    const double mm = mod_plain(word, m.ps);
    double k;
    const double rho = divmod_below_2p53(m.ps.rho * mm + m.ps.half, m.ps, &k);      // (Q mod t) m' + h < 2^41
    return mulmod_f64(m.ps.half - rho, m.tinv, p.qd, p.inv_qd);                       // |h - rho| < 2^20
}

// The opening's decode: residues x1 < q1, x2 < q2 of x in [0, Q) -> floor((t x + (Q - 1) / 2) / Q) mod t.
//   x1' = x1 mod q2                      one conditional subtraction (x1 < 2^44 < 2 q2)
//   y   = (x2 - x1') q1^-1 mod q2        Barrett product, y < q2
//   x   = x1 + q1 y                      < q1 + q1 (q2 - 1) = Q < 2^88          (128-bit)
//   N   = t x + (Q - 1) / 2              < 2^20 2^88 + 2^87 < 2^109             (128-bit)
//   s   = floor(N / Q) in [0, t]: estimated in FP64 as floor(t (y + x1 / q1) / q2 + 1/2) — a value below 2^21 with relative error
//         below 2^-50, so the estimate is off by at most one — and made exact by comparing N - s Q with 0 and Q (two fix-ups either
//         way, constant trip count; no 128-bit division exists on the device and none is needed)
//   slot = s mod t = (s == t ? 0 : s)
__device__ __forceinline__ uint64_t rns_decode_slot(uint64_t x1, uint64_t x2, const RnsConsts& rc, const ModParams& p2) {
    const uint64_t x1r = x1 >= rc.q[1] ? x1 - rc.q[1] : x1;
    const uint64_t diff = x2 >= x1r ? x2 - x1r : x2 + rc.q[1] - x1r;
    const uint64_t y = mulmod_barrett128(diff, rc.q1inv, p2);
    const unsigned __int128 big = ((unsigned __int128)rc.big_hi << 64) | rc.big_lo;
    const unsigned __int128 x = (unsigned __int128)rc.q[0] * y + x1;
    const unsigned __int128 num = x * rc.t + (big >> 1);
    const double est = (double)rc.t * (((double)y + (double)x1 * rc.inv_q1) * rc.inv_q2) + 0.5;
    uint64_t s = (uint64_t)(long long)__builtin_floor(est);
    s = s > rc.t ? rc.t : s;
    __int128 rem = (__int128)num - (__int128)((unsigned __int128)s * big);
#pragma unroll
    for (int fix = 0; fix < 2; ++fix) {
        const bool under = rem < 0;
        rem += under ? (__int128)big : (__int128)0;
        s -= under ? 1 : 0;
    }
#pragma unroll
    for (int fix = 0; fix < 2; ++fix) {
        const bool over = rem >= (__int128)big;
        rem -= over ? (__int128)big : (__int128)0;
        s += over ? 1 : 0;
    }
    return s == rc.t ? 0 : s;
}
// rns_decode_slot with the measured noise: after the fix-ups rem = N - s Q lies in [0, Q), and
// rho = |rem - (Q - 1) / 2| = |t x - s Q| <= (Q - 1) / 2 < 2^87 — its bit length comes from the two halves
__device__ __forceinline__ uint64_t rns_decode_slot_noise(uint64_t x1, uint64_t x2, const RnsConsts& rc, const ModParams& p2, uint32_t* rho_bits) {
    const uint64_t x1r = x1 >= rc.q[1] ? x1 - rc.q[1] : x1;
    const uint64_t diff = x2 >= x1r ? x2 - x1r : x2 + rc.q[1] - x1r;
    const uint64_t y = mulmod_barrett128(diff, rc.q1inv, p2);
    const unsigned __int128 big = ((unsigned __int128)rc.big_hi << 64) | rc.big_lo;
    const unsigned __int128 x = (unsigned __int128)rc.q[0] * y + x1;
    const unsigned __int128 num = x * rc.t + (big >> 1);
    const double est = (double)rc.t * (((double)y + (double)x1 * rc.inv_q1) * rc.inv_q2) + 0.5;
    uint64_t s = (uint64_t)(long long)__builtin_floor(est);
    s = s > rc.t ? rc.t : s;
    __int128 rem = (__int128)num - (__int128)((unsigned __int128)s * big);
#pragma unroll
    for (int fix = 0; fix < 2; ++fix) {
        const bool under = rem < 0;
        rem += under ? (__int128)big : (__int128)0;
        s -= under ? 1 : 0;
    }
#pragma unroll
    for (int fix = 0; fix < 2; ++fix) {
        const bool over = rem >= (__int128)big;
        rem -= over ? (__int128)big : (__int128)0;
        s += over ? 1 : 0;
    }
    const __int128 off = rem - (__int128)(big >> 1);
    const unsigned __int128 rho = (unsigned __int128)(off < 0 ? -off : off);
    const uint64_t rho_hi = (uint64_t)(rho >> 64), rho_lo = (uint64_t)rho;
    *rho_bits = rho_hi ? 64u + bitlen64(rho_hi) : bitlen64(rho_lo);
    return s == rc.t ? 0 : s;
}

// ---- elementwise kernels of "rns-general" ---------------------------------------------------------------------------------------
// v[j][x] = (v[j][x] + e2[j][x] + round(Q (msg[j][x] mod t) / t)) mod q_i for x < copy: the scalar component's epilogue under prime i
__global__ void __launch_bounds__(256) rns_finish_v_kernel(uint64_t* __restrict__ v, const uint64_t* __restrict__ e2, const uint64_t* __restrict__ msgs,
                                                             uint64_t msg_len, uint64_t copy, uint32_t logn, uint64_t count, RnsConsts rc, int prime,
                                                             ModParams p) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    const uint64_t nmask = (1ull << logn) - 1;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += stride) {
        const uint64_t x = i & nmask, j = i >> logn;
        uint64_t s = v[i] + e2[i];
        if (s >= p.q) s -= p.q;
        if (x < copy) {
            s += rns_message_term(msgs[j * msg_len + x], rc, prime, p);
            if (s >= p.q) s -= p.q;
        }
        v[i] = s;
    }
}

// residue block `prime` of the rows [batch][6 + 2 (kn + n)] from that prime's u and v (prime 0 also writes the header)
__global__ void __launch_bounds__(256) rns_pack_kernel(uint64_t* __restrict__ out, const uint64_t* __restrict__ u, const uint64_t* __restrict__ v, uint64_t kn,
                                                         uint64_t n, uint64_t batch, int prime, RnsConsts rc, uint64_t shape) {
    const uint64_t block = kn + n, words = kRnsHeaderWords + 2 * block;
    const uint64_t head = prime == 0 ? kRnsHeaderWords : 0, part = head + block;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < batch * part; i += stride) {
        const uint64_t j = i / part, w = i - j * part;
        uint64_t* const row = out + j * words;
        if (w < head) { row[w] = rns_header_word((uint32_t)w, words, shape, rc); continue; }
        const uint64_t b = w - head;
        row[kRnsHeaderWords + (uint64_t)prime * block + b] = b < kn ? u[j * kn + b] : v[j * n + (b - kn)];
    }
}

// the reverse, with the header check (prime 0) and the canonicity screening of that prime's block: bad[j] != 0 marks row j
__global__ void __launch_bounds__(256) rns_unpack_kernel(const uint64_t* __restrict__ rows, uint64_t* __restrict__ u, uint64_t* __restrict__ v,
                                                           uint32_t* __restrict__ bad, uint64_t kn, uint64_t n, uint64_t batch, int prime, RnsConsts rc,
                                                           uint64_t shape) {
    const uint64_t block = kn + n, words = kRnsHeaderWords + 2 * block;
    const uint64_t head = prime == 0 ? kRnsHeaderWords : 0, part = head + block;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < batch * part; i += stride) {
        const uint64_t j = i / part, w = i - j * part;
        const uint64_t* const row = rows + j * words;
        bool ok;
        if (w < head) {
            ok = row[w] == rns_header_word((uint32_t)w, words, shape, rc);
        } else {
            const uint64_t b = w - head, x = row[kRnsHeaderWords + (uint64_t)prime * block + b];
            if (b < kn) u[j * kn + b] = x;
            else v[j * n + (b - kn)] = x;
            ok = x < rc.q[prime];
        }
        if (!ok) atomicOr(&bad[j], 1u);
    }
}

// flags[j] |= OR_i decode(w1[j][i], w2[j][i]) xor msg[j][i], one lane per (j, i): w_p = v_p - <s, u_p> under prime p
__global__ void __launch_bounds__(256) rns_decode_compare_kernel(const uint64_t* __restrict__ w1, const uint64_t* __restrict__ w2,
                                                                   const uint64_t* __restrict__ msgs, uint64_t msg_len, uint32_t logn, uint64_t count,
                                                                   RnsConsts rc, ModParams p2, unsigned long long* __restrict__ flags) {
    const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= count * msg_len) return;
    const uint64_t j = gid / msg_len, i = gid - j * msg_len;
    const uint64_t diff = rns_decode_slot(w1[(j << logn) + i], w2[(j << logn) + i], rc, p2) ^ msgs[gid];
    if (diff) atomicOr(&flags[j], (unsigned long long)diff);
}
// the decoding twin, lanes as decode_store_batch_kernel: out[j][i] = decode(w1[j][i], w2[j][i]) for i < slots
template <bool NOISE>
__global__ void __launch_bounds__(256) rns_decode_store_kernel(const uint64_t* __restrict__ w1, const uint64_t* __restrict__ w2, uint64_t* __restrict__ out,
                                                                 uint64_t slots, uint32_t logn, uint64_t count, RnsConsts rc, ModParams p2,
                                                                 unsigned long long* __restrict__ noise) {
    const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if constexpr (NOISE) {
        const uint64_t j = gid >> logn, i = gid & ((1ull << logn) - 1);
        const bool live = j < count;
        uint32_t bits = 0;
        if (live) {
            const uint64_t slot = rns_decode_slot_noise(w1[gid], w2[gid], rc, p2, &bits);
            if (i < slots) out[j * slots + i] = slot;
        }
        if (logn >= 6) row_noise_max(&noise[live ? j : 0], bits);
        else if (live) atomicMax(&noise[j], (unsigned long long)bits);
    } else {
        if (gid >= count * slots) return;
        const uint64_t j = gid / slots, i = gid - j * slots;
        out[gid] = rns_decode_slot(w1[(j << logn) + i], w2[(j << logn) + i], rc, p2);
    }
}

// ---- "rns-tile" -----------------------------------------------------------------------------------------------------------------
// everything of one prime a tile pass needs
struct RnsTilePrime {
    const double* mat;           // [A^T | b_hat] (commit) or s_hat (open) in the lane-major layout of f8_permute_matrix_kernel
    ModParams p;
    const double* fwd_tw;
    const double* inv_tw;
    RoundConsts<ArithF64> cs;
};

#ifndef LSR_RNS_TILE_TW_REGS
#define LSR_RNS_TILE_TW_REGS 1   // the last round's multipliers in registers: 40 KB of LDS for the transform instead of 69 KB
#endif                           // (0: multipliers in LDS, one workgroup per CU, 256 VGPRs — the experiment build of DESIGN.md §6a)

// One stream block (eight consecutive coefficients, block number = lane) of the Gaussian object (key, domain, index), kept as
// signed 8-bit values in coefficient order: tables of <= 64 scanned entries give |sample| <= 63
__device__ __forceinline__ void f8_sample_to_keep(const uint64_t* __restrict__ key, uint32_t domain, uint32_t index, const LaneTable& tab, uint32_t entries,
                                                  int8_t* __restrict__ keep) {
    uint64_t w[8], u[8];
    stream_block(key, domain, index, threadIdx.x, w);
#pragma unroll
    for (int i = 0; i < 8; ++i) u[i] = w[i] >> 1;
    uint32_t magnitude[8];
    cdt_magnitudes(tab, nullptr, entries, u, magnitude);
    uint32_t packed[2] = {0u, 0u};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t a = magnitude[i];
        const uint32_t sa = (w[i] & 1ull) ? 0u - a : a;
        packed[i >> 2] |= (sa & 0xFFu) << (8 * (i & 3));
    }
    *reinterpret_cast<uint2*>(keep + 8 * threadIdx.x) = make_uint2(packed[0], packed[1]);
}

struct CommitRnsTileJob {
    uint64_t* rows;              // [batch][6 + 2 (k + 1) n] wire rows, device
    const uint64_t* keys;        // [batch][4] per-commitment stream keys
    const uint64_t* msgs;        // [batch][msg_len]; only read when copy > 0
    uint64_t msg_len, copy;
    const uint64_t* cdf;
    uint32_t entries;            // scanned entries (<= 64)
    uint32_t batch;
    RnsConsts rc;
};

// r_i: sampled in the first pass and left in LDS, read back in the second
template <bool SAMPLE>
struct CommitRnsTileSource {
    const uint64_t* key;
    LaneTable tab;
    uint32_t entries;
    int8_t* keep;                // [K][4096]
    __device__ __forceinline__ void load(int i, double (&v)[kF8Regs]) const {
        int8_t* const mine = keep + ((size_t)i << 12);
        if constexpr (SAMPLE) {
            f8_sample_to_keep(key, kDomR, (uint32_t)i, tab, entries, mine);
            __syncthreads();
        }
#pragma unroll
        for (int k = 0; k < kF8Regs; ++k) v[k] = (double)mine[threadIdx.x + 512u * (uint32_t)k];
    }
    __device__ __forceinline__ uint32_t ahead(int) const { return 0; }
};
// u_c = . + e1_c,  v = . + e2 + (round(Q (m mod t) / t) mod q_i): canonical words into residue block PRIME of the wire row;
// e1_c / e2 are sampled by the first pass into LDS and read back by the second
template <int K, int PRIME>
struct CommitRnsTileSink {
    const CommitRnsTileJob& job;
    const uint64_t* key;
    LaneTable tab;
    int8_t* keep;                // [K + 1][4096]
    uint64_t* block;             // this commitment's residue block of prime PRIME
    const uint64_t* msg;
    const ModParams& p;
    __device__ __forceinline__ void store(int c, const double (&x)[kF8Regs]) const {
        int8_t* const mine = keep + ((size_t)c << 12);
        if constexpr (PRIME == 0) {
            f8_sample_to_keep(key, c < K ? kDomE1 : kDomE2, c < K ? (uint32_t)c : 0u, tab, job.entries, mine);
            __syncthreads();
        }
        uint64_t* const dst = block + ((size_t)c << 12);
        const RnsPlainScale ps = make_rns_plain_scale(job.rc, PRIME);
#pragma unroll
        for (int k = 0; k < kF8Regs; ++k) {
            const uint32_t idx = threadIdx.x + 512u * (uint32_t)k;
            double v = x[k] + (double)mine[idx];
            if (c == K && idx < job.copy) v += rns_embed_plain(msg[idx], ps, p);    // |.| <= 0.875 q
            dst[idx] = u52_from_f64(canonical_f64(v, p.qd, p.inv_qd));              // |v| < 2 q + 2^7
        }
    }
};

template <int K>
__global__ void __launch_bounds__(kF8Threads, LSR_RNS_TILE_TW_REGS ? 4 : 2) commit_rns_tile_kernel(CommitRnsTileJob job, RnsTilePrime a, RnsTilePrime b) {
    constexpr bool TW = LSR_RNS_TILE_TW_REGS != 0;
    __shared__ double tile_lds[kF8TileWords];
    __shared__ double tw_lds[kF8TwShared + (TW ? 0 : kF8TwPrivate)];
    __shared__ __attribute__((aligned(16))) int8_t keep[(2 * K + 1) * 4096];     // r_0 .. r_{K-1}, e1_0 .. e1_{K-1}, e2
    const uint32_t j = blockIdx.x;
    if (j >= job.batch) return;
    const uint64_t* const key = job.keys + 4 * (size_t)j;
    const LaneTable tab = lane_table_load(job.cdf, job.entries);
    constexpr size_t block_words = (size_t)(K + 1) << 12, row_words = kRnsHeaderWords + 2 * block_words;
    uint64_t* const row = job.rows + (size_t)j * row_words;
    if (threadIdx.x < kRnsHeaderWords) row[threadIdx.x] = rns_header_word(threadIdx.x, row_words, 4096ull | ((uint64_t)K << 32), job.rc);
    const uint64_t* const msg = job.msgs + (size_t)j * job.msg_len;
    {
        CommitRnsTileSource<true> src{key, tab, job.entries, keep};
        CommitRnsTileSink<K, 0> sink{job, key, tab, keep + K * 4096, row + kRnsHeaderWords, msg, a.p};
        f8_tile_pipeline<K, K + 1, true, CommitRnsTileSource<true>, CommitRnsTileSink<K, 0>, TW>(0u, src, sink, a.mat, a.p, a.fwd_tw, a.inv_tw, a.cs, tile_lds,
                                                                                                 tw_lds);
    }
    __syncthreads();             // the first pass's last readers of the twiddle image and the tile are done
    {
        CommitRnsTileSource<false> src{key, tab, job.entries, keep};
        CommitRnsTileSink<K, 1> sink{job, key, tab, keep + K * 4096, row + kRnsHeaderWords + block_words, msg, b.p};
        f8_tile_pipeline<K, K + 1, true, CommitRnsTileSource<false>, CommitRnsTileSink<K, 1>, TW>(0u, src, sink, b.mat, b.p, b.fwd_tw, b.inv_tw, b.cs, tile_lds,
                                                                                                  tw_lds);
    }
}

// ---- openings ---------------------------------------------------------------------------------------------------------------------
struct VerifyRnsTileJob {
    const uint64_t* rows;        // [count][6 + 2 (k + 1) n]
    const uint64_t* msgs;        // [count][msg_len] claimed messages (raw words)
    uint64_t msg_len;            // 1 .. n
    unsigned long long* flags;   // [count]: OR over the slots of decoded ^ claimed
    uint32_t* bad;               // [count]: != 0 when the row is not a canonical commitment of this context
    uint32_t count;
    RnsConsts rc;
};
// u_i of one residue block: canonical words -> elements; a word >= q_p marks the row
struct VerifyRnsTileSource {
    const uint64_t* block;
    uint32_t* bad;
    uint64_t q;
    __device__ __forceinline__ void load(int i, double (&v)[kF8Regs]) const {
        const uint64_t* const src = block + ((size_t)i << 12);
        bool ok = true;
#pragma unroll
        for (int k = 0; k < kF8Regs; ++k) {
            const uint64_t raw = src[threadIdx.x + 512u * (uint32_t)k];
            ok = ok && raw < q;
            v[k] = f64_from_u52(raw);
        }
        if (!ok) atomicOr(bad, 1u);
    }
    // the next polynomial of the block (after the last u_i: v, which the sink reads) towards this XCD's L2, as VerifyTileSource does
    __device__ __forceinline__ uint32_t ahead(int i) const {
        if (threadIdx.x < 256) {
            const rsrc_t nxt = make_rsrc(block + ((size_t)(i + 1) << 12), 4096u * 8u);
            return __builtin_amdgcn_raw_buffer_load_b32(nxt, (int)(threadIdx.x * 128u), 0, 0);
        }
        return 0;
    }
};
// w_p = v_p - INTT(<s_hat, u_hat>) mod q_p.  The first pass leaves w_1 in registers; the second lifts (w_1, w_2) to [0, Q), decodes
// slot by slot and compares with the claimed words as given
template <int K, int PRIME>
struct VerifyRnsTileSink {
    const VerifyRnsTileJob& job;
    const uint64_t* vsrc;        // v of this prime's block
    const uint64_t* msg;
    unsigned long long* flag;
    uint32_t* bad;
    const ModParams& p;
    double (&w1)[kF8Regs];
    __device__ __forceinline__ void store(int, const double (&x)[kF8Regs]) const {
        uint64_t diff = 0;
        bool ok = true;
#pragma unroll
        for (int k = 0; k < kF8Regs; ++k) {
            const uint32_t idx = threadIdx.x + 512u * (uint32_t)k;
            const uint64_t raw = vsrc[idx];
            ok = ok && raw < p.q;
            const double w = canonical_f64(f64_from_u52(raw) - x[k], p.qd, p.inv_qd);
            if constexpr (PRIME == 0) {
                w1[k] = w;
            } else {
                if (idx < job.msg_len) diff |= rns_decode_slot(u52_from_f64(w1[k]), u52_from_f64(w), job.rc, p) ^ msg[idx];
            }
        }
        if (!ok) atomicOr(bad, 1u);
        if (diff) atomicOr(flag, (unsigned long long)diff);
    }
};

template <int K>
__global__ void __launch_bounds__(kF8Threads, 4) verify_rns_tile_kernel(VerifyRnsTileJob job, RnsTilePrime a, RnsTilePrime b) {
    __shared__ double tile_lds[kF8TileWords];
    __shared__ double tw_lds[kF8TwShared];
    const uint32_t j = blockIdx.x;
    if (j >= job.count) return;
    constexpr size_t block_words = (size_t)(K + 1) << 12, row_words = kRnsHeaderWords + 2 * block_words;
    const uint64_t* const row = job.rows + (size_t)j * row_words;
    if (threadIdx.x < kRnsHeaderWords && row[threadIdx.x] != rns_header_word(threadIdx.x, row_words, 4096ull | ((uint64_t)K << 32), job.rc))
        atomicOr(&job.bad[j], 1u);
    const uint64_t* const msg = job.msgs + (size_t)j * job.msg_len;
    double w1[kF8Regs];
    {
        const uint64_t* const block = row + kRnsHeaderWords;
        VerifyRnsTileSource src{block, &job.bad[j], job.rc.q[0]};
        VerifyRnsTileSink<K, 0> sink{job, block + ((size_t)K << 12), msg, &job.flags[j], &job.bad[j], a.p, w1};
        f8_tile_pipeline<K, 1, true, VerifyRnsTileSource, VerifyRnsTileSink<K, 0>, true>(0u, src, sink, a.mat, a.p, a.fwd_tw, a.inv_tw, a.cs, tile_lds, tw_lds);
    }
    __syncthreads();
    {
        const uint64_t* const block = row + kRnsHeaderWords + block_words;
        VerifyRnsTileSource src{block, &job.bad[j], job.rc.q[1]};
        VerifyRnsTileSink<K, 1> sink{job, block + ((size_t)K << 12), msg, &job.flags[j], &job.bad[j], b.p, w1};
        f8_tile_pipeline<K, 1, true, VerifyRnsTileSource, VerifyRnsTileSink<K, 1>, true>(0u, src, sink, b.mat, b.p, b.fwd_tw, b.inv_tw, b.cs, tile_lds, tw_lds);
    }
}

// ---- decoding -------------------------------------------------------------------------------------------------------
struct DecodeRnsTileJob {
    const uint64_t* rows;        // [count][6 + 2 (k + 1) n]
    uint64_t* out;               // [count][slots] decoded plaintext slots
    uint64_t slots;              // 1 .. n
    unsigned long long* noise;   // [count]: max over the row's coefficients of bitlen(rho) (NOISE only)
    uint32_t* bad;
    uint32_t count;
    RnsConsts rc;
};
// as VerifyRnsTileSink: the first pass leaves w_1 in registers, the second lifts, decodes and stores the slots
template <int K, int PRIME, bool NOISE>
struct DecodeRnsTileSink {
    const DecodeRnsTileJob& job;
    const uint64_t* vsrc;        // v of this prime's block
    uint64_t* out;
    unsigned long long* noise;
    uint32_t* bad;
    const ModParams& p;
    double (&w1)[kF8Regs];
    __device__ __forceinline__ void store(int, const double (&x)[kF8Regs]) const {
        uint32_t bits = 0;
        bool ok = true;
#pragma unroll
        for (int k = 0; k < kF8Regs; ++k) {
            const uint32_t idx = threadIdx.x + 512u * (uint32_t)k;
            const uint64_t raw = vsrc[idx];
            ok = ok && raw < p.q;
            const double w = canonical_f64(f64_from_u52(raw) - x[k], p.qd, p.inv_qd);
            if constexpr (PRIME == 0) {
                w1[k] = w;
            } else if constexpr (NOISE) {
                uint32_t b;
                const uint64_t slot = rns_decode_slot_noise(u52_from_f64(w1[k]), u52_from_f64(w), job.rc, p, &b);
                bits = b > bits ? b : bits;
                if (idx < job.slots) out[idx] = slot;
            } else {
                if (idx < job.slots) out[idx] = rns_decode_slot(u52_from_f64(w1[k]), u52_from_f64(w), job.rc, p);
            }
        }
        if (!ok) atomicOr(bad, 1u);
        if constexpr (PRIME == 1 && NOISE) row_noise_max(noise, bits);
    }
};

template <int K, bool NOISE>
__global__ void __launch_bounds__(kF8Threads, 4) decode_rns_tile_kernel(DecodeRnsTileJob job, RnsTilePrime a, RnsTilePrime b) {
    __shared__ double tile_lds[kF8TileWords];
    __shared__ double tw_lds[kF8TwShared];
    const uint32_t j = blockIdx.x;
    if (j >= job.count) return;
    constexpr size_t block_words = (size_t)(K + 1) << 12, row_words = kRnsHeaderWords + 2 * block_words;
    const uint64_t* const row = job.rows + (size_t)j * row_words;
    if (threadIdx.x < kRnsHeaderWords && row[threadIdx.x] != rns_header_word(threadIdx.x, row_words, 4096ull | ((uint64_t)K << 32), job.rc))
        atomicOr(&job.bad[j], 1u);
    uint64_t* const out = job.out + (size_t)j * job.slots;
    double w1[kF8Regs];
    {
        const uint64_t* const block = row + kRnsHeaderWords;
        VerifyRnsTileSource src{block, &job.bad[j], job.rc.q[0]};
        DecodeRnsTileSink<K, 0, NOISE> sink{job, block + ((size_t)K << 12), out, &job.noise[j], &job.bad[j], a.p, w1};
        f8_tile_pipeline<K, 1, true, VerifyRnsTileSource, DecodeRnsTileSink<K, 0, NOISE>, true>(0u, src, sink, a.mat, a.p, a.fwd_tw, a.inv_tw, a.cs, tile_lds, tw_lds);
    }
    __syncthreads();
    {
        const uint64_t* const block = row + kRnsHeaderWords + block_words;
        VerifyRnsTileSource src{block, &job.bad[j], job.rc.q[1]};
        DecodeRnsTileSink<K, 1, NOISE> sink{job, block + ((size_t)K << 12), out, &job.noise[j], &job.bad[j], b.p, w1};
        f8_tile_pipeline<K, 1, true, VerifyRnsTileSource, DecodeRnsTileSink<K, 1, NOISE>, true>(0u, src, sink, b.mat, b.p, b.fwd_tw, b.inv_tw, b.cs, tile_lds, tw_lds);
    }
}

}  // namespace lsr
