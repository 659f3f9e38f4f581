// Kernels of the batched prove_r1cs / verify_r1cs path (lsr_prover.hip): polynomial evaluation over the Goldilocks
// field, the commitment message, the proof records and the verifier's per-proof check.
#pragma once

#include <cstdint>

#include "lsr_arith.hpp"

namespace lsr {

constexpr int kEvalBlock = 256;
constexpr int kEvalRows = 512;                 // table rows per pass: 512 x 256 = 2^17 coefficients
constexpr int kEvalPass = kEvalRows * kEvalBlock;
constexpr uint64_t kGoldOneMont = kGoldEpsilon;   // 1 in Montgomery form (2^64 mod p)

__device__ __forceinline__ uint64_t gold_canonical(uint64_t x) { return x >= kGoldilocks ? x - kGoldilocks : x; }

// up to three polynomials per instance with the same layout: poly[j][inst * stride + pos], pos < len
struct EvalPolys {
    const uint64_t* poly[3];
    size_t stride;
    uint32_t len;
};
// point k of instance i (k < count): x[k & 1][i * stride + 2 * blockIdx.y]; blockIdx.y walks the pairs
struct EvalPoints {
    const uint64_t* x[2];
    size_t stride;
    uint32_t count;
};
// value of polynomial j at point k of instance i: v[i * inst_stride + j * poly_stride + 2 * blockIdx.y + k]
struct EvalOut {
    uint64_t* v;
    size_t inst_stride, poly_stride;
};

__device__ __forceinline__ uint32_t rev_bits(uint32_t v, int bits) { return bits ? __brev(v) >> (32 - bits) : 0u; }

// sum_pos (c_pos mod p) x^e(pos) mod p for NPOLY polynomials of one instance and up to two points, one workgroup each.
//   NATURAL (BITREV = false): e(pos) = pos — the quotient and eval_poly;
//   BITREV:                   e(pos) = bitrev_logm(pos), len = m = 2^logm — the planes the quotient plan's forward transform
//                             leaves (m P coeffs), scaled back by `scale_mont` = m^-1 (Montgomery form).
// Lane t reads the coefficients pos = r 256 + t (coalesced rows), so x^e(pos) = f_t * T[r]: f_t depends on the lane only and the
// table T (LDS, one entry per row, broadcast reads) on the row only.  One Montgomery product per coefficient and point; the
// lane's sum is multiplied by f_t once and the workgroup adds its 256 partial sums.  The sums are exact residues: any order
// gives the same words.
// More than 2^17 coefficients are walked in PASSES of 512 rows that reuse the table: row r = pass 512 + rr, and
//   NATURAL: e = t + (rr << 8) + (pass << 17)                                          -> f_t T[rr] (x^(2^17))^pass;
//   BITREV:  e = rev8(t) << (logm - 8) | rev9(rr) << (logm - 17) | rev_{logm-17}(pass)  -> f_t T[rr] x^rev(pass).
// eval_partial covers the rows [row0, row0 + row_count) that exist (whole passes or a part of one) and returns, in lanes
// t < 2 NPOLY, the workgroup's unscaled sum of polynomial t >> 1 at point t & 1.
template <bool BITREV, int NPOLY>
__device__ __forceinline__ uint64_t eval_partial(const EvalPolys& polys, const EvalPoints& pts, int logm, uint32_t row0, uint32_t row_count) {
    __shared__ uint64_t table[2][kEvalRows];
    __shared__ uint64_t partial[kEvalBlock / 64][NPOLY][2];
    const size_t inst = blockIdx.x;
    const int t = threadIdx.x;
    const uint32_t first = 2u * blockIdx.y;
    const int npts = (pts.count - first) >= 2 ? 2 : 1;
    const uint32_t len = polys.len;
    const uint32_t rows = (len + kEvalBlock - 1) / kEvalBlock;
    // BITREV: pos = r 256 + t with lo = min(logm, 8) bits of lane and hi = logm - lo bits of row, of which the top pass_bits count passes
    const int lo_bits = logm < 8 ? logm : 8, hi_bits = logm - lo_bits;
    const int pass_bits = BITREV && hi_bits > 9 ? hi_bits - 9 : 0, row_bits = hi_bits - pass_bits;
    const int exp_bits = BITREV && logm > 17 ? logm : 17;
    uint64_t lane_f[2], step[2], xm[2];   // step: x^(2^17) for the natural order's passes; xm: x (both Montgomery)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const uint64_t raw = k < npts ? pts.x[k][inst * pts.stride + first] : 0;
        uint64_t sq = gold_mul(gold_canonical(raw), kGoldEpsilon);   // x^(2^b) in Montgomery form, b = 0, 1, ...
        xm[k] = sq;
        uint64_t f = kGoldOneMont, e0 = kGoldOneMont, e1 = kGoldOneMont;
        const uint32_t lane_exp = BITREV ? (rev_bits((uint32_t)t & ((1u << lo_bits) - 1u), lo_bits) << hi_bits) : (uint32_t)t;
        const uint32_t r0 = (uint32_t)t, r1 = (uint32_t)t + kEvalBlock;
        const uint32_t x0 = BITREV ? rev_bits(r0, row_bits) << pass_bits : r0 << 8, x1 = BITREV ? rev_bits(r1, row_bits) << pass_bits : r1 << 8;
        for (int b = 0; b < exp_bits; ++b) {
            if ((lane_exp >> b) & 1u) f = gold_mul_mont(f, sq);
            if ((x0 >> b) & 1u) e0 = gold_mul_mont(e0, sq);
            if ((x1 >> b) & 1u) e1 = gold_mul_mont(e1, sq);
            if (b == 16) step[k] = gold_mul_mont(sq, sq);      // x^(2^17)
            sq = gold_mul_mont(sq, sq);
        }
        lane_f[k] = f;
        table[k][r0] = e0;
        table[k][r1] = e1;
    }
    __syncthreads();
    uint64_t total[NPOLY][2];
#pragma unroll
    for (int j = 0; j < NPOLY; ++j) total[j][0] = total[j][1] = 0;
    uint64_t pass_f[2] = {kGoldOneMont, kGoldOneMont};         // NATURAL: (x^(2^17))^pass
    if (!BITREV) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            uint64_t sq = step[k];
            for (uint32_t e = row0 / (uint32_t)kEvalRows; e; e >>= 1) {
                if (e & 1u) pass_f[k] = gold_mul_mont(pass_f[k], sq);
                sq = gold_mul_mont(sq, sq);
            }
        }
    }
    const uint32_t row_end = (row0 >= rows || row_count > rows - row0) ? rows : row0 + row_count;
    for (uint32_t pass = row0 / (uint32_t)kEvalRows; pass * (uint32_t)kEvalRows < row_end && row0 < row_end; ++pass) {
        const uint32_t base = pass * (uint32_t)kEvalRows;
        const uint32_t begin = base > row0 ? base : row0;
        const uint32_t end = row_end - base < (uint32_t)kEvalRows ? row_end : base + kEvalRows;
        uint64_t acc[NPOLY][2];
#pragma unroll
        for (int j = 0; j < NPOLY; ++j) acc[j][0] = acc[j][1] = 0;
        for (uint32_t r = begin; r < end; ++r) {
            const uint32_t pos = r * kEvalBlock + (uint32_t)t;
            const uint64_t w0 = table[0][r - base], w1 = table[1][r - base];
            if (pos < len) {
#pragma unroll
                for (int j = 0; j < NPOLY; ++j) {
                    const uint64_t c = polys.poly[j][inst * polys.stride + pos];
                    acc[j][0] = gold_add(acc[j][0], gold_mul_mont(c, w0));
                    acc[j][1] = gold_add(acc[j][1], gold_mul_mont(c, w1));
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            uint64_t pf = pass_f[k];
            if (BITREV) {                                      // x^rev(pass): pass_bits <= 5 squarings
                pf = kGoldOneMont;
                uint64_t sq = xm[k];
                const uint32_t e = rev_bits(pass, pass_bits);
                for (int b = 0; b < pass_bits; ++b) {
                    if ((e >> b) & 1u) pf = gold_mul_mont(pf, sq);
                    sq = gold_mul_mont(sq, sq);
                }
            }
            const uint64_t g = gold_mul_mont(lane_f[k], pf);
#pragma unroll
            for (int j = 0; j < NPOLY; ++j) total[j][k] = gold_add(total[j][k], gold_mul_mont(acc[j][k], g));
            pass_f[k] = gold_mul_mont(pass_f[k], step[k]);
        }
    }
    // workgroup sum: wave shuffles, then one partial per wave through LDS
#pragma unroll
    for (int j = 0; j < NPOLY; ++j)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            uint64_t v = total[j][k];
            for (int off = 32; off; off >>= 1) {
                const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off);
                v = gold_add(v, ((uint64_t)hi << 32) | lo);
            }
            if ((t & 63) == 0) partial[t >> 6][j][k] = v;
        }
    __syncthreads();
    uint64_t v = 0;
    if (t < NPOLY * 2) {
        const int j = t >> 1, k = t & 1;
#pragma unroll
        for (int w = 0; w < kEvalBlock / 64; ++w) v = gold_add(v, partial[w][j][k]);
    }
    return v;
}

// one workgroup walks every pass of its polynomials (grid: instances x point pairs)
template <bool BITREV, int NPOLY>
__global__ void __launch_bounds__(kEvalBlock) eval_kernel(EvalPolys polys, EvalPoints pts, EvalOut out, int logm, uint64_t scale_mont) {
    const uint64_t v = eval_partial<BITREV, NPOLY>(polys, pts, logm, 0u, ~0u);
    const int t = threadIdx.x;
    const uint32_t first = 2u * blockIdx.y;
    if (t < NPOLY * 2 && first + (uint32_t)(t & 1) < pts.count)
        out.v[blockIdx.x * out.inst_stride + (size_t)(t >> 1) * out.poly_stride + first + (t & 1)] = gold_mul_mont(v, scale_mont);
}

// Long polynomials in few instances (m > 2^17: a chunk of the prove call holds 16 instances or fewer at m = 2^22): the passes are
// spread over gridDim.z slices of `rows_per_slice` 256-coefficient rows each (gridDim.y already walks the point pairs; a slice may be a
// part of a pass: the m = 4096 workload runs 16 rows per workgroup the same way), every slice leaves its sums in
// part[((inst pairs + pair) slices + slice)][NPOLY][2], and eval_combine_kernel adds the slices and scales.  Exact residues: the same
// words as the single-workgroup walk.
template <bool BITREV, int NPOLY>
__global__ void __launch_bounds__(kEvalBlock) eval_slice_kernel(EvalPolys polys, EvalPoints pts, uint64_t* __restrict__ part, int logm,
                                                                uint32_t rows_per_slice) {
    const uint64_t v = eval_partial<BITREV, NPOLY>(polys, pts, logm, blockIdx.z * rows_per_slice, rows_per_slice);
    const size_t cell = ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * gridDim.z + blockIdx.z;
    if (threadIdx.x < NPOLY * 2) part[cell * (NPOLY * 2) + threadIdx.x] = v;
}
// one lane per (instance, point pair, polynomial, point of the pair)
template <int NPOLY>
__global__ void __launch_bounds__(256) eval_combine_kernel(const uint64_t* __restrict__ part, uint32_t pairs, uint32_t slices, uint32_t count,
                                                           EvalOut out, uint64_t scale_mont, size_t lanes) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= lanes) return;
    const uint32_t jk = (uint32_t)(i % (NPOLY * 2));
    const size_t cell = i / (NPOLY * 2);                       // inst pairs + pair
    const size_t inst = cell / pairs;
    const uint32_t first = 2u * (uint32_t)(cell - inst * pairs);
    if (first + (jk & 1u) >= count) return;
    uint64_t v = 0;
    for (uint32_t s = 0; s < slices; ++s) v = gold_add(v, part[(cell * slices + s) * (NPOLY * 2) + jk]);
    out.v[inst * out.inst_stride + (size_t)(jk >> 1) * out.poly_stride + first + (jk & 1u)] = gold_mul_mont(v, scale_mont);
}

// the commitment message of prove_r1cs / prove_r1cs_zk: msg[i][j] = Q'_j mod commit_modulus, Q' = Q + r (X^m - 1) built as poly_add
// builds it (r1cs.rs:906-922; coefficient 0 takes Q_0 - r, coefficient m takes r); blinding == nullptr: Q' = Q
__global__ void __launch_bounds__(256) prove_message_kernel(const uint64_t* __restrict__ quot, uint32_t m, const uint64_t* __restrict__ blinding,
                                                            uint64_t commit_modulus, uint64_t* __restrict__ msg, uint32_t msg_len, size_t total) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        const size_t i = idx / msg_len;
        const uint32_t j = (uint32_t)(idx - i * msg_len);
        uint64_t v = j < m ? quot[i * m + j] : 0;
        if (blinding) {
            const uint64_t r = gold_canonical(blinding[i]);
            if (j == 0) v = gold_sub(v, r);
            if (j == m) v = r;
        }
        msg[idx] = v % commit_modulus;
    }
}

// public_inputs(witness) = witness[0..n_public] (raw words), gathered contiguously for the transcript kernel
__global__ void __launch_bounds__(256) gather_publics_kernel(const uint64_t* __restrict__ z, uint32_t n_vars, uint32_t n_public,
                                                             uint64_t* __restrict__ out, size_t total) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        const size_t i = idx / n_public;
        out[idx] = z[i * n_vars + (idx - i * n_public)];
    }
}

__device__ __forceinline__ uint64_t gold_pow2k(uint64_t x, int logm) {   // x^(2^logm), x canonical
    for (int b = 0; b < logm; ++b) x = gold_mul(x, x);
    return x;
}

// one lane per instance: the proof record (ProofR1CS / ProofR1csZk field order, prover.h), status and the two transcript hashes.
// ev[i][8] = A(alpha) A(beta) B(alpha) B(beta) C(alpha) C(beta) Q(alpha) Q(beta).
__global__ void __launch_bounds__(256) prove_assemble_kernel(const uint64_t* __restrict__ ev, const uint64_t* __restrict__ alphas,
                                                             const uint64_t* __restrict__ betas, const uint64_t* __restrict__ blinding,
                                                             const uint32_t* __restrict__ len, const uint64_t* __restrict__ hash_a,
                                                             const uint64_t* __restrict__ hash_b, int logm, uint64_t* __restrict__ proofs,
                                                             uint64_t* __restrict__ hashes, uint32_t* __restrict__ status, size_t count) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint64_t* e = ev + i * 8;
    const uint64_t alpha = alphas[i], beta = betas[i];
    uint64_t qa = e[6], qb = e[7], r = 0;
    if (blinding) {   // Q'(x) = Q(x) + r (x^m - 1): the same residue eval_poly gives on the coefficients of Q'
        r = gold_canonical(blinding[i]);
        qa = gold_add(qa, gold_mul(r, gold_sub(gold_pow2k(alpha, logm), 1)));
        qb = gold_add(qb, gold_mul(r, gold_sub(gold_pow2k(beta, logm), 1)));
    }
    uint64_t* p = proofs + i * 13;
    p[0] = alpha;  p[1] = beta;  p[2] = qa;   p[3] = qb;
    p[4] = e[0];   p[5] = e[2];  p[6] = e[4];
    p[7] = e[1];   p[8] = e[3];  p[9] = e[5];
    p[10] = qa;    p[11] = qb;   p[12] = r;
    status[i] = len[i];
    if (hashes) {
        for (int w = 0; w < 4; ++w) {
            hashes[i * 8 + w] = hash_a[i * 4 + w];
            hashes[i * 8 + 4 + w] = hash_b[i * 4 + w];
        }
    }
}

// ---- verify_r1cs / verify_r1cs_zk (lib.rs:1016-1095, 1142-1215) with the u64/u128 semantics of arith.rs:8-37 for ANY input word ----
constexpr uint64_t kVerifyModulus = 0xFFFFFFFF00000001ull;

__host__ __device__ inline uint64_t vfy_mul_mod(uint64_t a, uint64_t b) {   // (a b mod p), any 64-bit a, b
#ifdef __HIP_DEVICE_COMPILE__
    return gold_mul(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) % kVerifyModulus);
#endif
}
__host__ __device__ inline uint64_t vfy_sub_mod(uint64_t a, uint64_t b) {   // wrapping u128: a + p - b, minus p once if >= p
    unsigned __int128 d = (unsigned __int128)a + kVerifyModulus - (unsigned __int128)b;
    if (d >= kVerifyModulus) d -= kVerifyModulus;
    return (uint64_t)d;
}
__host__ __device__ inline uint64_t vfy_pow(uint64_t x, uint64_t e) {       // mod_pow (arith.rs:42-61): base %= p first
    uint64_t base = x >= kVerifyModulus ? x - kVerifyModulus : x, r = 1;
    while (e) {
        if (e & 1) r = vfy_mul_mod(r, base);
        base = vfy_mul_mod(base, base);
        e >>= 1;
    }
    return r;
}
// alpha_re / beta_re: the transcripts recomputed from (public inputs, row) and ([alpha_re], row) — beta is derived from the
// proof's alpha only once that equals alpha_re, so deriving it from alpha_re is the same
__host__ __device__ inline int verify_one(const uint64_t* p, uint64_t alpha_re, uint64_t beta_re, uint32_t m, bool zk) {
    if (p[0] != alpha_re || p[1] != beta_re) return 0;
    const uint64_t x[2] = {p[0], p[1]};
    for (int k = 0; k < 2; ++k) {
        const uint64_t zh = vfy_sub_mod(vfy_pow(x[k], m), 1);   // eval_vanishing (r1cs.rs:424-429)
        uint64_t q = p[2 + k];
        if (zk) q = vfy_sub_mod(q, vfy_mul_mod(p[12], zh));
        const uint64_t lhs = vfy_mul_mod(q, zh);
        const uint64_t rhs = vfy_sub_mod(vfy_mul_mod(p[4 + 3 * k], p[5 + 3 * k]), p[6 + 3 * k]);
        if (lhs != rhs) return 0;
    }
    return (p[10] == p[2] && p[11] == p[3]) ? 1 : 0;
}

__global__ void __launch_bounds__(256) verify_check_kernel(const uint64_t* __restrict__ proofs, const uint64_t* __restrict__ alphas,
                                                           const uint64_t* __restrict__ betas, uint32_t m, int zk, int* __restrict__ results,
                                                           size_t count) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) results[i] = verify_one(proofs + i * 13, alphas[i], betas[i], m, zk != 0);
}

}  // namespace lsr
