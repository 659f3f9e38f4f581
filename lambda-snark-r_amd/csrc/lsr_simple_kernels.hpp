// Kernels of the witness-polynomial proofs (lsr_simple.hip): the message pass (witness mod q, plus the
// ChaCha20Rng blinding of random_blinding, into the opening coefficients f' and the commit message f' mod commit_modulus), the
// evaluation f'(alpha) that also writes the proof record, and the checks of verify_simple.  Arithmetic: MontQ, any odd q < 2^64.
#pragma once

#include <cstdint>

#include "lsr_montq.hpp"
#include "lsr_sampler.hpp"

namespace lsr {

constexpr int kSimpleBlock = 256;
// L <= 64: one lane per instance evaluates f' by sequential Horner (L products); longer polynomials take one wavefront each (Horner
// in x^64 per lane, then 6 squarings, up to 6 products for x^t and a 6-step reduction: about 20 products per lane whatever L is,
// so below 64 coefficients a wavefront per instance would do 20x the work with 60 lanes or more idle)
constexpr uint32_t kSimpleLaneMaxL = 64;
enum SimpleMode : int { kSimplePlain = 0, kSimpleZk = 1, kSimpleSimulate = 2 };

// ---- the message pass: one lane per 8 consecutive coefficients of one instance (= one ChaCha20 block of its blinding) ------------
// ChaCha20Rng (rand_chacha 0.3.1) with key k, stream 0: u64 draw j is 64-bit word j % 8 of the RFC 8439 block with counter j / 8
// and nonce 0, which is stream_block(k, 0, 0, j / 8).  MODE kSimplePlain: f'_j = w_j mod q; kSimpleZk: add_mod(w_j mod q, r_j);
// kSimpleSimulate: f'_j = r_j (w unread); r_j = draw j mod q.  coeffs [count][len] receives f'; msg (may be null) [count][msg_len]
// receives f' mod commit_modulus for j < msg_len.
template <int MODE>
__global__ void __launch_bounds__(kSimpleBlock) simple_message_kernel(const uint64_t* __restrict__ w, const uint64_t* __restrict__ keys,
                                                                      uint64_t* __restrict__ coeffs, uint64_t* __restrict__ msg, uint32_t len,
                                                                      uint32_t msg_len, uint64_t commit_modulus, size_t total, MontQ M) {
    const uint32_t groups = (len + 7) / 8;
    const size_t stride = (size_t)gridDim.x * kSimpleBlock;
    for (size_t g = (size_t)blockIdx.x * kSimpleBlock + threadIdx.x; g < total; g += stride) {
        const size_t inst = g / groups;
        const uint32_t c0 = (uint32_t)(g - inst * groups) * 8;
        const uint32_t live = len - c0 < 8u ? len - c0 : 8u;
        uint64_t r[8];
        if constexpr (MODE != kSimplePlain) {
            const uint64_t key[4] = {keys[inst * 4], keys[inst * 4 + 1], keys[inst * 4 + 2], keys[inst * 4 + 3]};
            stream_block(key, 0, 0, c0 / 8, r);
        }
        const size_t at = inst * len + c0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if ((uint32_t)j >= live) break;
            uint64_t v;
            if constexpr (MODE == kSimpleSimulate) {
                v = mq_canon(r[j], M);
            } else {
                v = mq_canon(w[at + j], M);
                if constexpr (MODE == kSimpleZk) v = mq_add(v, mq_canon(r[j], M), M);
            }
            coeffs[at + j] = v;
            if (msg && c0 + j < msg_len) msg[inst * msg_len + c0 + j] = v >= commit_modulus ? v % commit_modulus : v;
        }
    }
}

// ---- evaluation: Polynomial::evaluate (polynomial.rs:97-113) ----------------------------------------------------------------------
// REDUCE: coefficients are any 64-bit words, taken mod q first (verify: Field::new(c % modulus)); else they are already canonical.
template <bool REDUCE>
__host__ __device__ inline uint64_t simple_coef(const uint64_t* c, size_t j, const MontQ& M) {
    return REDUCE ? mq_canon(c[j], M) : c[j];
}
// sequential Horner, the reference's own order; 0 for len = 0
template <bool REDUCE>
__host__ __device__ inline uint64_t simple_horner(const uint64_t* c, uint32_t len, uint64_t x, const MontQ& M) {
    if (len == 0) return 0;
    const uint64_t xm = mq_to(x, M);
    uint64_t acc = simple_coef<REDUCE>(c, len - 1, M);
    for (uint32_t j = len - 1; j-- > 0;) acc = mq_add(mq_mul(acc, xm, M), simple_coef<REDUCE>(c, j, M), M);
    return acc;
}
// one wavefront: lane t sums c_{64 r + t} x^{64 r} by Horner in x^64, multiplies by x^t, and an xor butterfly adds the 64 partial
// sums (every lane ends with the total).  Every step is exact in canonical residues: the same word as sequential Horner.
template <bool REDUCE>
__device__ inline uint64_t simple_horner_wave(const uint64_t* c, uint32_t len, uint64_t x, const MontQ& M) {
    const uint32_t t = threadIdx.x & 63u;
    const uint64_t xm = mq_to(x, M);
    uint64_t x64 = xm, xt = M.r1;                        // Montgomery forms of x^64 and x^t
    for (int b = 0; b < 6; ++b) {
        if ((t >> b) & 1) xt = mq_mul(xt, x64, M);
        x64 = mq_mul(x64, x64, M);
    }
    uint64_t acc = 0;
    const uint32_t rows = len > t ? (len - 1 - t) / 64 + 1 : 0;
    for (uint32_t r = rows; r-- > 0;) acc = mq_add(mq_mul(acc, x64, M), simple_coef<REDUCE>(c, (size_t)r * 64 + t, M), M);
    acc = mq_mul(acc, xt, M);
    for (int off = 32; off; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)acc, off), hi = (uint32_t)__shfl_xor((int)(uint32_t)(acc >> 32), off);
        acc = mq_add(acc, ((uint64_t)hi << 32) | lo, M);
    }
    return acc;
}

// prove: f'(alpha) and the record {alpha, evaluation, seed} (generate_opening, opening.rs:104-115).  WAVE: one wavefront per instance
// (4 per block), else one lane per instance.
template <bool WAVE>
__global__ void __launch_bounds__(kSimpleBlock) simple_eval_kernel(const uint64_t* __restrict__ coeffs, uint32_t len,
                                                                   const uint64_t* __restrict__ alphas, const uint64_t* __restrict__ seeds,
                                                                   uint64_t* __restrict__ proofs, size_t count, MontQ M) {
    const size_t inst = WAVE ? (size_t)blockIdx.x * (kSimpleBlock / 64) + threadIdx.x / 64 : (size_t)blockIdx.x * kSimpleBlock + threadIdx.x;
    if (inst >= count) return;                           // uniform per wavefront in the WAVE form
    const uint64_t a = alphas[inst];
    const uint64_t* c = coeffs + inst * len;
    uint64_t y;
    if constexpr (WAVE) y = simple_horner_wave<false>(c, len, a, M);
    else y = simple_horner<false>(c, len, a, M);
    if (WAVE && (threadIdx.x & 63u)) return;
    uint64_t* p = proofs + inst * 3;
    p[0] = a;
    p[1] = y;
    p[2] = seeds[inst];
}

// verify_simple (lib.rs:1269-1285 with verify_opening, opening.rs:229-264): alpha as raw words, evaluation < q, len >= 1, Horner
__host__ __device__ inline int simple_verdict(const uint64_t* p, uint64_t alpha_re, uint64_t horner, uint32_t len, const MontQ& M) {
    return (p[0] == alpha_re && p[1] < M.q && len >= 1 && horner == p[1]) ? 1 : 0;
}
template <bool WAVE>
__global__ void __launch_bounds__(kSimpleBlock) simple_check_kernel(const uint64_t* __restrict__ proofs, const uint64_t* __restrict__ coeffs,
                                                                    uint32_t len, const uint64_t* __restrict__ alphas, int* __restrict__ results,
                                                                    size_t count, MontQ M) {
    const size_t inst = WAVE ? (size_t)blockIdx.x * (kSimpleBlock / 64) + threadIdx.x / 64 : (size_t)blockIdx.x * kSimpleBlock + threadIdx.x;
    if (inst >= count) return;
    const uint64_t* p = proofs + inst * 3;
    const uint64_t* c = coeffs + inst * len;
    uint64_t y;
    if constexpr (WAVE) y = simple_horner_wave<true>(c, len, p[0], M);
    else y = simple_horner<true>(c, len, p[0], M);
    if (WAVE && (threadIdx.x & 63u)) return;
    results[inst] = simple_verdict(p, alphas[inst], y, len, M);
}

// the claimed message of verify_opening_with_context (opening.rs:198-201): (c mod q) mod commit_modulus, [count][len]
__global__ void __launch_bounds__(kSimpleBlock) simple_claim_kernel(const uint64_t* __restrict__ coeffs, uint64_t* __restrict__ msg,
                                                                    uint64_t commit_modulus, size_t total, MontQ M) {
    const size_t stride = (size_t)gridDim.x * kSimpleBlock;
    for (size_t i = (size_t)blockIdx.x * kSimpleBlock + threadIdx.x; i < total; i += stride) {
        const uint64_t v = mq_canon(coeffs[i], M);
        msg[i] = v >= commit_modulus ? v % commit_modulus : v;
    }
}

// results[i] &= (lwe_verify_opening == 1); opened == nullptr (len > ring degree: the reference's call returns 0 or -1): results = 0
__global__ void __launch_bounds__(kSimpleBlock) simple_and_kernel(int* __restrict__ results, const int* __restrict__ opened, size_t count) {
    const size_t i = (size_t)blockIdx.x * kSimpleBlock + threadIdx.x;
    if (i < count) results[i] = (results[i] == 1 && opened && opened[i] == 1) ? 1 : 0;
}

}  // namespace lsr
