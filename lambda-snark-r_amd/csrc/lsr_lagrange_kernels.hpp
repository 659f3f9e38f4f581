// Kernels of the Lagrange (baseline) prove path (lsr_lagrange.hip), on the Montgomery arithmetic of lsr_montq.hpp:
// the batched interpolation GEMM against the plan's resident L, the top half of A B, the Toeplitz quotient, the remainder test of
// the omega domain, the commitment message, polynomial evaluation, the proof records and the generic-modulus verifier.
#pragma once

#include <cstdint>

#include "lsr_arith.hpp"
#include "lsr_montq.hpp"

namespace lsr {

// ---- wide accumulator: sum of 128-bit products in 192 bits, one reduction per output -----------------------------------------
// Every sum below has at most m <= 8192 products of canonical words, so it is < 2^13 q^2 < 2^141: t2 < 2^13, nothing overflows.
struct Acc192 {
    uint64_t t0, t1, t2;
};
__host__ __device__ inline void acc_zero(Acc192& a) { a.t0 = a.t1 = a.t2 = 0; }
__host__ __device__ inline void acc_mac(Acc192& a, uint64_t x, uint64_t y) {
    const uint64_t lo = x * y, hi = mq_mulhi(x, y);   // hi <= 2^64 - 2: hi + 1 does not wrap
    a.t0 += lo;
    const uint64_t h = hi + (a.t0 < lo ? 1u : 0u);
    a.t1 += h;
    a.t2 += a.t1 < h ? 1u : 0u;
}
// S 2^-128 mod q, canonical, for S = t2:t1:t0 with t2 < 2^13: two REDC steps.  The first leaves U = S 2^-64 = u1:u0 with
// u1 <= t2 + 1; the second V = u1 + mulhi(t1', q) + [u0 != 0] < q + t2 + 2, which is < 2q once q > 2^14, else < 2^15.
__host__ __device__ inline uint64_t acc_reduce(const Acc192& a, const MontQ& M) {
    uint64_t t = a.t0 * M.qinv;
    uint64_t th = mq_mulhi(t, M.q) + (a.t0 != 0 ? 1u : 0u);   // mulhi <= q - 1 < 2^64 - 1
    uint64_t u0 = a.t1 + th;
    const uint64_t u1 = a.t2 + (u0 < th ? 1u : 0u);
    t = u0 * M.qinv;
    th = mq_mulhi(t, M.q);
    uint64_t v = u1 + th;
    bool carry = v < th;
    const uint64_t c = u0 != 0 ? 1u : 0u;
    v += c;
    carry |= v < c;
    if (carry || v >= M.q) v -= M.q;
    if (v >= M.q) v %= M.q;                                  // q < 2^15 only
    return v;
}

constexpr int kLagBlock = 256;

// ---- constraint evaluations for a generic modulus (SparseMatrix::mul_vec, sparse_matrix.rs:259-289) --------------------------
struct LagCsr {
    const uint32_t* row_ptr;   // [m + 1]
    const uint32_t* col;
    const uint64_t* val;       // val mod q in Montgomery form (val 2^64 mod q): z val~ 2^-64 = (z mod q)(val mod q) for any 64-bit z
};
__global__ void __launch_bounds__(kLagBlock) lag_constraint_evals_kernel(uint64_t* __restrict__ out, LagCsr a, LagCsr b, LagCsr c,
                                                                         const uint64_t* __restrict__ z, uint32_t n_vars, uint32_t m,
                                                                         size_t per_vector, MontQ M) {
    const LagCsr mat = blockIdx.y == 0 ? a : (blockIdx.y == 1 ? b : c);
    const size_t stride = (size_t)gridDim.x * kLagBlock;
    for (size_t i = (size_t)blockIdx.x * kLagBlock + threadIdx.x; i < per_vector; i += stride) {
        const size_t inst = i / m;
        const uint32_t row = (uint32_t)(i - inst * m);
        const uint64_t* zi = z + inst * n_vars;
        uint64_t acc = 0;
        for (uint32_t e = mat.row_ptr[row]; e < mat.row_ptr[row + 1]; ++e) acc = mq_add(acc, mq_mul(zi[mat.col[e]], mat.val[e], M), M);
        out[blockIdx.y * per_vector + i] = acc;
    }
}

// is_satisfied (r1cs.rs:148-172): bad[inst] |= a b != c
__global__ void __launch_bounds__(kLagBlock) lag_check_kernel(const uint64_t* __restrict__ a, const uint64_t* __restrict__ b,
                                                              const uint64_t* __restrict__ c, uint32_t* __restrict__ bad, uint32_t m,
                                                              size_t per_vector, MontQ M) {
    const size_t stride = (size_t)gridDim.x * kLagBlock;
    for (size_t i = (size_t)blockIdx.x * kLagBlock + threadIdx.x; i < per_vector; i += stride)
        if (mq_mul(mq_mul(a[i], b[i], M), M.r2, M) != c[i]) atomicOr(&bad[i / m], 1u);
}

// ---- interpolation: coef[r][k] = sum_i e[r][i] L[k][i], r < rows (= 3 instances), k < m ------------------------------------
// lt = L^T scaled by 2^128: lt[i * m + k] = L[k][i] 2^128 mod q, so the reduction's 2^-128 leaves the coefficient itself.
// m > 64: 64 x 64 output tiles, 256 lanes of 4 x 4 outputs, K in blocks of 16 through LDS (evaluations stored k-major so a lane's
// four rows are broadcast reads, L rows are 16 consecutive words per 16 lanes).
constexpr int kGemmTile = 64, kGemmK = 16;
__global__ void __launch_bounds__(kLagBlock) lag_interp_tiled_kernel(const uint64_t* __restrict__ e, const uint64_t* __restrict__ lt,
                                                                     uint64_t* __restrict__ coef, size_t rows, uint32_t m, MontQ M) {
    __shared__ uint64_t es[kGemmK][kGemmTile + 1];
    __shared__ uint64_t ls[kGemmK][kGemmTile];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const size_t r0 = (size_t)blockIdx.x * kGemmTile;
    const uint32_t c0 = blockIdx.y * kGemmTile;
    Acc192 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc_zero(acc[a][b]);
    for (uint32_t k0 = 0; k0 < m; k0 += kGemmK) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {   // 64 rows x 16 k of evaluations, 64 cols x 16 k of L^T
            const int idx = j * kLagBlock + t;
            const int er = idx >> 4, ek = idx & 15;
            const size_t gr = r0 + er;
            const uint32_t gk = k0 + ek;
            es[ek][er] = (gr < rows && gk < m) ? e[gr * m + gk] : 0;
            const int lk = idx >> 6, lc = idx & 63;
            const uint32_t gi = k0 + lk, gc = c0 + lc;
            ls[lk][lc] = (gi < m && gc < m) ? lt[(size_t)gi * m + gc] : 0;
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < kGemmK; ++kk) {
            uint64_t x[4], y[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) x[a] = es[kk][ty + 16 * a];
#pragma unroll
            for (int b = 0; b < 4; ++b) y[b] = ls[kk][tx + 16 * b];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc_mac(acc[a][b], x[a], y[b]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const size_t gr = r0 + ty + 16 * a;
        if (gr >= rows) continue;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint32_t gc = c0 + tx + 16 * b;
            if (gc < m) coef[gr * m + gc] = acc_reduce(acc[a][b], M);
        }
    }
}

// m <= 64: the whole L^T (<= 32 KiB) and 64 evaluation rows (<= 32 KiB) in LDS; the block's 64 m outputs are dealt to its lanes
// in order, so a wave covers 64 / m instances' rows at once (the reference's benchmark sizes m = 10 ... 64)
constexpr int kSmallRows = 64, kSmallMaxM = 64;
__global__ void __launch_bounds__(kLagBlock) lag_interp_small_kernel(const uint64_t* __restrict__ e, const uint64_t* __restrict__ lt,
                                                                     uint64_t* __restrict__ coef, size_t rows, uint32_t m, MontQ M) {
    __shared__ uint64_t ls[kSmallMaxM * kSmallMaxM];
    __shared__ uint64_t es[kSmallRows * kSmallMaxM];
    const int t = threadIdx.x;
    const size_t r0 = (size_t)blockIdx.x * kSmallRows;
    const uint32_t live_rows = (uint32_t)(rows - r0 < (size_t)kSmallRows ? rows - r0 : kSmallRows);
    const uint32_t mm = m * m, outs = live_rows * m;
    for (uint32_t i = t; i < mm; i += kLagBlock) ls[i] = lt[i];
    for (uint32_t i = t; i < outs; i += kLagBlock) es[i] = e[r0 * m + i];   // rows are contiguous: one linear run
    __syncthreads();
    for (uint32_t o = t; o < outs; o += kLagBlock) {
        const uint32_t r = o / m, k = o - r * m;
        Acc192 acc;
        acc_zero(acc);
        for (uint32_t i = 0; i < m; ++i) acc_mac(acc, es[r * m + i], ls[i * m + k]);
        coef[r0 * m + o] = acc_reduce(acc, M);
    }
}

// ---- quotient --------------------------------------------------------------------------------------------------------------
// top[inst][j] = coefficient m + j of A B (j < m - 1): sum_{s = j+1}^{m-1} A_s B_{m+j-s}.  C has degree < m and does not enter.
__global__ void __launch_bounds__(kLagBlock) lag_top_kernel(const uint64_t* __restrict__ A, const uint64_t* __restrict__ B,
                                                            uint64_t* __restrict__ top, uint32_t m, size_t total, MontQ M) {
    const uint32_t w = m - 1;
    const size_t stride = (size_t)gridDim.x * kLagBlock;
    for (size_t idx = (size_t)blockIdx.x * kLagBlock + threadIdx.x; idx < total; idx += stride) {
        const size_t inst = idx / w;
        const uint32_t j = (uint32_t)(idx - inst * w);
        const uint64_t* a = A + inst * m;
        const uint64_t* b = B + inst * m;
        Acc192 acc;
        acc_zero(acc);
        for (uint32_t s = j + 1; s < m; ++s) acc_mac(acc, a[s], b[m + j - s]);
        top[idx] = mq_mul(acc_reduce(acc, M), M.r3, M);       // S 2^-128 -> S
    }
}

// Q = floor(N / Z_H) through the reversed polynomials: rev(Q) = rev(N) / rev(Z_H) mod X^(m-1), i.e.
// Q_j = sum_{d=j}^{m-2} top_d T_{d-j}, T = the power series of 1 / rev(Z_H) (tser = T 2^128).  quot[inst][j] for j < m (the last
// word, and the only one when m = 1, is 0).
__global__ void __launch_bounds__(kLagBlock) lag_toeplitz_kernel(const uint64_t* __restrict__ top, const uint64_t* __restrict__ tser,
                                                                 uint64_t* __restrict__ quot, uint32_t m, size_t total, MontQ M) {
    const uint32_t w = m - 1;
    const size_t stride = (size_t)gridDim.x * kLagBlock;
    for (size_t idx = (size_t)blockIdx.x * kLagBlock + threadIdx.x; idx < total; idx += stride) {
        const size_t inst = idx / m;
        const uint32_t j = (uint32_t)(idx - inst * m);
        const uint64_t* tp = top + inst * w;
        Acc192 acc;
        acc_zero(acc);
        for (uint32_t d = j; d < w; ++d) acc_mac(acc, tp[d], tser[d - j]);
        quot[idx] = acc_reduce(acc, M);
    }
}

// the omega domain only: N mod Z_H = 0, coefficient by coefficient below m:  (A B)_k - C_k = (Q Z_H)_k for k < m.
// zh_s = Z_H 2^128.  A failing coefficient marks the instance.
__global__ void __launch_bounds__(kLagBlock) lag_remainder_kernel(const uint64_t* __restrict__ A, const uint64_t* __restrict__ B,
                                                                  const uint64_t* __restrict__ C, const uint64_t* __restrict__ quot,
                                                                  const uint64_t* __restrict__ zh_s, uint32_t* __restrict__ bad, uint32_t m,
                                                                  size_t total, MontQ M) {
    const size_t stride = (size_t)gridDim.x * kLagBlock;
    for (size_t idx = (size_t)blockIdx.x * kLagBlock + threadIdx.x; idx < total; idx += stride) {
        const size_t inst = idx / m;
        const uint32_t k = (uint32_t)(idx - inst * m);
        const uint64_t* a = A + inst * m;
        const uint64_t* b = B + inst * m;
        const uint64_t* qq = quot + inst * m;
        Acc192 ab, qz;
        acc_zero(ab);
        acc_zero(qz);
        for (uint32_t s = 0; s <= k; ++s) acc_mac(ab, a[s], b[k - s]);
        const uint32_t jend = k < m - 1 ? k + 1 : m - 1;      // j <= k and Q_j = 0 for j >= m - 1
        for (uint32_t j = 0; j < jend; ++j) acc_mac(qz, qq[j], zh_s[k - j]);
        const uint64_t lhs = mq_sub(mq_mul(acc_reduce(ab, M), M.r3, M), C[idx], M);
        if (lhs != acc_reduce(qz, M)) atomicOr(&bad[inst], 1u);
    }
}

// per instance: the quotient length (trailing zeros trimmed, >= 1; compute_quotient_poly) or 0 when the witness failed
__global__ void __launch_bounds__(kLagBlock) lag_len_kernel(const uint64_t* __restrict__ quot, const uint32_t* __restrict__ bad,
                                                            uint32_t* __restrict__ len, uint32_t m, size_t count) {
    const size_t i = (size_t)blockIdx.x * kLagBlock + threadIdx.x;
    if (i >= count) return;
    uint32_t l = m;
    while (l > 1 && quot[i * m + l - 1] == 0) --l;
    len[i] = bad[i] ? 0u : l;
}

// Q' = Q (+ r Z_H, poly_add of r1cs.rs:906-922 with the dense Z_H) mod q into qp [count][m + 1]; msg = Q' mod commit_modulus
// [count][msg_len].  zh_m = Z_H 2^64 (r Z_H = mq_mul(r, zh_m)); blinding == nullptr: Q' = Q.
__global__ void __launch_bounds__(kLagBlock) lag_message_kernel(const uint64_t* __restrict__ quot, const uint64_t* __restrict__ blinding,
                                                                const uint64_t* __restrict__ zh_m, uint64_t* __restrict__ qp,
                                                                uint64_t* __restrict__ msg, uint32_t msg_len, uint64_t commit_modulus,
                                                                uint32_t m, size_t total, MontQ M) {
    const size_t stride = (size_t)gridDim.x * kLagBlock;
    for (size_t idx = (size_t)blockIdx.x * kLagBlock + threadIdx.x; idx < total; idx += stride) {
        const size_t i = idx / (m + 1);
        const uint32_t j = (uint32_t)(idx - i * (m + 1));
        uint64_t v = j < m ? quot[i * m + j] : 0;
        if (blinding) v = mq_add(v, mq_mul(blinding[i] % M.q, zh_m[j], M), M);
        qp[idx] = v;
        if (j < msg_len) msg[i * msg_len + j] = v % commit_modulus;
    }
}

// public_inputs(witness) = witness[0..n_public] (raw words), gathered for the transcript kernel
__global__ void __launch_bounds__(kLagBlock) lag_gather_publics_kernel(const uint64_t* __restrict__ z, uint32_t n_vars, uint32_t n_public,
                                                                       uint64_t* __restrict__ out, size_t total) {
    const size_t stride = (size_t)gridDim.x * kLagBlock;
    for (size_t idx = (size_t)blockIdx.x * kLagBlock + threadIdx.x; idx < total; idx += stride) {
        const size_t i = idx / n_public;
        out[idx] = z[i * n_vars + (idx - i * n_public)];
    }
}

// eval_poly (r1cs.rs:362-373) of up to four polynomials per instance at alpha and beta: one wave per (instance, polynomial).
// Lane t takes coefficients t, t + 64, ... by Horner in x^64 (Montgomery form, one product per coefficient and point), then
// multiplies by x^t and the wave adds its 64 partial sums.  ev[inst][8]: A(a) A(b) B(a) B(b) C(a) C(b) Q'(a) Q'(b).
struct LagEvalPolys {
    const uint64_t* poly[4];
    size_t stride[4];
    uint32_t len[4];
};
__global__ void __launch_bounds__(64) lag_eval_kernel(LagEvalPolys P, const uint64_t* __restrict__ alphas, const uint64_t* __restrict__ betas,
                                                      uint64_t* __restrict__ ev, MontQ M) {
    const size_t inst = blockIdx.x;
    const int j = blockIdx.y, t = threadIdx.x;
    const uint64_t* c = P.poly[j] + inst * P.stride[j];
    const uint32_t len = P.len[j];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const uint64_t x = k ? betas[inst] : alphas[inst];
        const uint64_t xm = mq_to(x, M);
        uint64_t x64 = xm, xt = M.r1;                        // Montgomery forms of x^64 and x^t
        for (int b = 0; b < 6; ++b) {
            if ((t >> b) & 1) xt = mq_mul(xt, x64, M);
            x64 = mq_mul(x64, x64, M);
        }
        uint64_t acc = 0;
        const uint32_t rows = len > (uint32_t)t ? (len - 1 - t) / 64 + 1 : 0;
        for (uint32_t r = rows; r-- > 0;) acc = mq_add(mq_mul(acc, x64, M), c[(size_t)r * 64 + t], M);
        acc = mq_mul(acc, xt, M);
        for (int off = 32; off; off >>= 1) {
            const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)acc, off), hi = (uint32_t)__shfl_xor((int)(uint32_t)(acc >> 32), off);
            acc = mq_add(acc, ((uint64_t)hi << 32) | lo, M);
        }
        if (t == 0) ev[inst * 8 + 2 * j + k] = acc;
    }
}

// one lane per instance: the proof record (prover.h LSR_PROOF_* order), status and the two transcript hashes
__global__ void __launch_bounds__(kLagBlock) lag_assemble_kernel(const uint64_t* __restrict__ ev, const uint64_t* __restrict__ alphas,
                                                                 const uint64_t* __restrict__ betas, const uint64_t* __restrict__ blinding,
                                                                 const uint32_t* __restrict__ len, const uint64_t* __restrict__ hash_a,
                                                                 const uint64_t* __restrict__ hash_b, uint64_t* __restrict__ proofs,
                                                                 uint64_t* __restrict__ hashes, uint32_t* __restrict__ status, size_t count,
                                                                 uint64_t q) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint64_t* e = ev + i * 8;
    uint64_t* p = proofs + i * 13;
    p[0] = alphas[i]; p[1] = betas[i]; p[2] = e[6]; p[3] = e[7];
    p[4] = e[0];      p[5] = e[2];     p[6] = e[4];
    p[7] = e[1];      p[8] = e[3];     p[9] = e[5];
    p[10] = e[6];     p[11] = e[7];    p[12] = blinding ? blinding[i] % q : 0;
    status[i] = len[i];
    if (hashes) {
        for (int w = 0; w < 4; ++w) {
            hashes[i * 8 + w] = hash_a[i * 4 + w];
            hashes[i * 8 + 4 + w] = hash_b[i * 4 + w];
        }
    }
}

// ---- verify_r1cs / verify_r1cs_zk for any modulus (lib.rs:1016-1095, 1142-1215), arith.rs:8-37 on ANY 64-bit proof word ----
// mul_mod = (a b) mod q in u128; add / sub in u128 with one conditional subtraction (sub_mod wraps as Rust's release u128).
__host__ __device__ inline uint64_t gv_mul(uint64_t a, uint64_t b, const MontQ& M) {   // any a, b
    return mq_mul(a % M.q, mq_to(b, M), M);
}
__host__ __device__ inline uint64_t gv_sub(uint64_t a, uint64_t b, uint64_t q) {
    unsigned __int128 d = (unsigned __int128)a + q - (unsigned __int128)b;
    if (d >= q) d -= q;
    return (uint64_t)d;
}
// eval_vanishing of the baseline path: prod_{i<m} sub_mod(x, i mod q)
__host__ __device__ inline uint64_t gv_vanishing(uint64_t x, uint32_t m, const MontQ& M) {
    uint64_t r = 1 % M.q;
    for (uint32_t i = 0; i < m; ++i) r = gv_mul(r, gv_sub(x, (uint64_t)i % M.q, M.q), M);
    return r;
}
__host__ __device__ inline int verify_one_generic(const uint64_t* p, uint64_t alpha_re, uint64_t beta_re, uint32_t m, bool zk, const MontQ& M) {
    if (p[0] != alpha_re || p[1] != beta_re) return 0;
    for (int k = 0; k < 2; ++k) {
        const uint64_t zh = gv_vanishing(p[k], m, M);
        uint64_t qv = p[2 + k];
        if (zk) qv = gv_sub(qv, gv_mul(p[12], zh, M), M.q);
        const uint64_t lhs = gv_mul(qv, zh, M);
        const uint64_t rhs = gv_sub(gv_mul(p[4 + 3 * k], p[5 + 3 * k], M), p[6 + 3 * k], M.q);
        if (lhs != rhs) return 0;
    }
    return (p[10] == p[2] && p[11] == p[3]) ? 1 : 0;
}

__global__ void __launch_bounds__(kLagBlock) lag_verify_kernel(const uint64_t* __restrict__ proofs, const uint64_t* __restrict__ alphas,
                                                               const uint64_t* __restrict__ betas, uint32_t m, int zk, int* __restrict__ results,
                                                               size_t count, MontQ M) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) results[i] = verify_one_generic(proofs + i * 13, alphas[i], betas[i], m, zk != 0, M);
}

}  // namespace lsr
