/*
 * lambda_snark/prover.h — ADDITIVE entry points for the prover-side polynomial path:
 * the cyclic NTT of rust-api/lambda-snark/src/ntt.rs and the NTT-path quotient polynomial of
 * rust-api/lambda-snark/src/r1cs.rs:474-506, on the same MI355X butterfly kernels as ntt.h.
 *
 * The reference computes these in Rust on the host (there is no C symbol to replace); a maintainer binds
 * them from `lagrange_interpolate_ntt` (r1cs.rs:772-793) and `compute_quotient_poly` — INTEGRATION.md §6.
 * Field: F_q with q = NTT_MODULUS = 2^64 - 2^32 + 1 and its 2^32-th root NTT_PRIMITIVE_ROOT
 * (rust-api/lambda-snark-core/src/lib.rs:58,78); other primes q < 2^61 work for the transforms.
 */
#pragma once

#include "lambda_snark/ntt.h"
#include "lambda_snark/r1cs.h"
#include "lambda_snark/types.h"

#ifdef __cplusplus
extern "C" {
#endif

/* NTT_MODULUS and NTT_PRIMITIVE_ROOT (lambda-snark-core/src/lib.rs:58,78) */
uint64_t lsr_prover_modulus(void) LSR_NOEXCEPT;
uint64_t lsr_prover_root_2_32(void) LSR_NOEXCEPT;
/* compute_root_of_unity(n, NTT_MODULUS, NTT_PRIMITIVE_ROOT) (ntt.rs:226-233); 0 unless n = 2^k <= 2^32 */
uint64_t lsr_prover_root_of_unity(uint64_t n) LSR_NOEXCEPT;

/* Context for cyclic transforms of size n = 2^k in [2, 131072] over prime q with omega a primitive n-th root
 * (omega = 0: the reference's root, q must then be NTT_MODULUS).  device -1 = default.  Free with ntt_context_free.
 * The ntt.h / batch.h transforms accept such a context and then run the cyclic butterfly network in its
 * native order: forward = natural in -> bit-reversed out, inverse = bit-reversed in -> natural out. */
NttContext* lsr_cyclic_ntt_context_create(uint64_t q, uint32_t n, uint64_t omega, int device) LSR_NOEXCEPT;
/* log2 of the largest transform size / constraint count of the *_large constructors and of lsr_r1cs_prover_create[_mod]: 22 */
uint32_t lsr_prover_max_log2_size(void) LSR_NOEXCEPT;
/* The same contract with n = 2^k in [2, 2^22]; at n <= 131072 it builds what lsr_cyclic_ntt_context_create builds.  Above 131072 the
 * transform runs three passes (two strided rounds and the tile pass) and q must be NTT_MODULUS: the FP64 and Shoup
 * flavours of the other primes are not carried through the extra round, so such a q returns NULL with a text in lsr_last_error.
 * Every transform entry point (ntt_forward/inverse[_batch], lsr_ntt_*_batch_device, lsr_cyclic_ntt_*_batch) takes the context;
 * lsr_ntt_ring_mul_batch[_device] returns -1 on a context above 131072.  One context holds two tables of n words and 3 n words of
 * staging on the device (160 MiB at n = 2^22). */
NttContext* lsr_cyclic_ntt_context_create_large(uint64_t q, uint32_t n, uint64_t omega, int device) LSR_NOEXCEPT;
int lsr_ntt_context_is_cyclic(const NttContext* ctx) LSR_NOEXCEPT;

/* ntt_forward / ntt_inverse of ntt.rs:117-201 for `batch` contiguous vectors of ctx->n words, natural order in
 * and out, host buffers, in place.  Inputs must be < q.  0 / -1. */
int lsr_cyclic_ntt_forward_batch(const NttContext* ctx, uint64_t* values, size_t batch) LSR_NOEXCEPT;
int lsr_cyclic_ntt_inverse_batch(const NttContext* ctx, uint64_t* values, size_t batch) LSR_NOEXCEPT;
/* device-resident bit-reversal of `batch` vectors of 2^logn words (d_out != d_in), asynchronous on `stream` */
int lsr_bit_reverse_device(uint64_t* d_out, const uint64_t* d_in, int logn, size_t batch, void* stream) LSR_NOEXCEPT;

/* ---- quotient polynomial Q = (A*B - C) / (X^m - 1) on the NTT path (r1cs.rs:386-389: m = 2^k, q = NTT_MODULUS) ---- */
typedef struct LsrQuotientPlan LsrQuotientPlan;
/* m = number of constraints, a power of two in [1, 131072]; NULL otherwise or without a GPU */
LsrQuotientPlan* lsr_quotient_plan_create(uint32_t m, int device) LSR_NOEXCEPT;
/* the same with m a power of two in [1, 2^22] (lsr_prover_max_log2_size); at m <= 131072 it builds what lsr_quotient_plan_create
 * builds.  Workspace: three planes of chunk * m words, chunk = min(batch, 2^26 / m) instances per pass (16 at m = 2^22: 1.5 GiB),
 * plus one plane for the quotient in the host call. */
LsrQuotientPlan* lsr_quotient_plan_create_large(uint32_t m, int device) LSR_NOEXCEPT;
void lsr_quotient_plan_free(LsrQuotientPlan* plan) LSR_NOEXCEPT;
uint32_t lsr_quotient_plan_size(const LsrQuotientPlan* plan) LSR_NOEXCEPT;
/* `batch` independent instances.  a/b/c_evals = [batch][m] constraint evaluations (A z, B z, C z of
 * compute_constraint_evals, r1cs.rs:296-304), values < q.  quotient = [batch][m] receives the coefficients of Q
 * (zero padded); quotient_len[i] = the length compute_quotient_poly would return (trailing zeros trimmed, >= 1), or 0
 * when the division leaves a remainder — the reference's Err "remainder non-zero (witness invalid)" (r1cs.rs:1050-1054);
 * the m quotient words of such an instance are unspecified.  Host buffers.  0 / -1. */
int lsr_quotient_batch(LsrQuotientPlan* plan, const uint64_t* a_evals, const uint64_t* b_evals, const uint64_t* c_evals,
                       size_t batch, uint64_t* quotient, uint32_t* quotient_len) LSR_NOEXCEPT;
/* same on device-resident buffers, asynchronous on `stream`; d_quotient [batch][m], d_quotient_len [batch].  A plan owns one
 * workspace: the library runs the calls on one plan one behind the other whatever streams they are given (a call waits on the
 * host for the previous asynchronous call's last kernel before it enqueues — use one plan per stream for concurrency); the
 * first call of a given batch size allocates, so make it outside a stream capture. */
int lsr_quotient_batch_device(LsrQuotientPlan* plan, const uint64_t* d_a_evals, const uint64_t* d_b_evals,
                              const uint64_t* d_c_evals, size_t batch, uint64_t* d_quotient, uint32_t* d_quotient_len,
                              void* stream) LSR_NOEXCEPT;

/* ---- compute_quotient_poly(witness) in full, for one R1CS and many witnesses (r1cs.rs:474-506) ----
 * The three sparse products of compute_constraint_evals (r1cs.rs:296-304, SparseMatrix::mul_vec sparse_matrix.rs:259-289:
 * values and witness words reduced mod q as unsigned integers) run on the device in front of the pipeline above.
 * A, B, C: m x n_vars in the FFI's coordinate form (r1cs.h; duplicate (row, col) entries add up), m = 2^k in [1, 2^22]
 * (lsr_prover_max_log2_size), modulus NTT_MODULUS.  The matrices are copied; NULL on bad shapes / indices or without a GPU.
 * Device memory of a prove call: 7 planes of chunk * m words (3 of the quotient plan, A's and B's interpolants, the quotient, the
 * commitment message), chunk = min(batch, 2^26 / m) — a peak of 3.5 GiB from m = 2^22 (16 instances per pass) down to any m with
 * batch * m >= 2^26; a quotient longer than the LWE ring degree is committed truncated to it, as lwe_commit truncates. */
typedef struct LsrR1csProver LsrR1csProver;
LsrR1csProver* lsr_r1cs_prover_create(const SparseMatrix* A, const SparseMatrix* B, const SparseMatrix* C, int device) LSR_NOEXCEPT;
void     lsr_r1cs_prover_free(LsrR1csProver* prover) LSR_NOEXCEPT;
uint32_t lsr_r1cs_prover_num_constraints(const LsrR1csProver* prover) LSR_NOEXCEPT;
uint32_t lsr_r1cs_prover_num_variables(const LsrR1csProver* prover) LSR_NOEXCEPT;
/* witnesses = [batch][n_vars] (host).  a/b/c_evals = [batch][m] receive A z, B z, C z (compute_constraint_evals). 0 / -1. */
int lsr_r1cs_constraint_evals_batch(LsrR1csProver* prover, const uint64_t* witnesses, size_t batch, uint64_t* a_evals,
                                    uint64_t* b_evals, uint64_t* c_evals) LSR_NOEXCEPT;
/* quotient / quotient_len as in lsr_quotient_batch; quotient_len[i] = 0 <=> witness i does not satisfy the R1CS
 * (is_satisfied, r1cs.rs:148-172 — the reference's Err "Witness does not satisfy R1CS constraints"). 0 / -1. */
int lsr_r1cs_quotient_batch(LsrR1csProver* prover, const uint64_t* witnesses, size_t batch, uint64_t* quotient,
                            uint32_t* quotient_len) LSR_NOEXCEPT;

/* ---- prove_r1cs / prove_r1cs_zk and verify_r1cs / verify_r1cs_zk for a batch of witnesses (lib.rs:747-809, 877-980,
 * 1016-1095, 1142-1215), NTT path only ----
 * One proof = LSR_R1CS_PROOF_WORDS uint64 words in ProofR1CS / ProofR1csZk field order (the commitment is the separate row). */
enum {
    LSR_PROOF_ALPHA, LSR_PROOF_BETA, LSR_PROOF_Q_ALPHA, LSR_PROOF_Q_BETA,
    LSR_PROOF_A_ALPHA, LSR_PROOF_B_ALPHA, LSR_PROOF_C_ALPHA,
    LSR_PROOF_A_BETA, LSR_PROOF_B_BETA, LSR_PROOF_C_BETA,
    LSR_PROOF_OPEN_ALPHA, LSR_PROOF_OPEN_BETA, LSR_PROOF_BLINDING, LSR_R1CS_PROOF_WORDS
};
/* witnesses [batch][n_vars]; seeds [batch] (0 = fresh OS entropy, as lwe_commit); blinding [batch] or NULL (NULL = prove_r1cs,
 * else prove_r1cs_zk with r = blinding[i] mod q).  Out: rows [batch][lsr_lwe_commitment_words(lwe)] = lwe_commit of the
 * (blinded) quotient reduced mod commit_modulus (Rust's LweContext::modulus()); proofs [batch][LSR_R1CS_PROOF_WORDS];
 * hashes [batch][2][32] (the transcripts of alpha and beta, may be NULL); status [batch] = the quotient length, or 0 when
 * witness i does not satisfy the R1CS (its row and proof words are then unspecified).  Host arrays, chunked staging.  0 / -1. */
int lsr_r1cs_prove_batch(LsrR1csProver* prover, LweContext* lwe, uint64_t commit_modulus, const uint64_t* witnesses, size_t batch,
                         size_t n_public, const uint64_t* seeds, const uint64_t* blinding, uint64_t* rows, uint64_t* proofs,
                         uint8_t* hashes, uint32_t* status) LSR_NOEXCEPT;
/* the same on device arrays on the prover's device, asynchronous on `stream`; `seeds` stays a HOST array and every seed must be
 * non-zero (-1 otherwise, as lsr_lwe_commit_keys_device).  Not capturable into a HIP graph (-1). */
int lsr_r1cs_prove_batch_device(LsrR1csProver* prover, LweContext* lwe, uint64_t commit_modulus, const uint64_t* d_witnesses,
                                size_t batch, size_t n_public, const uint64_t* seeds, const uint64_t* d_blinding, uint64_t* d_rows,
                                uint64_t* d_proofs, uint8_t* d_hashes, uint32_t* d_status, void* stream) LSR_NOEXCEPT;
/* verify_r1cs (zk = 0) / verify_r1cs_zk (zk != 0) of `batch` proofs of one circuit with m constraints (a power of two):
 * public_inputs [batch][n_public], rows [batch][words_per_row], proofs [batch][LSR_R1CS_PROOF_WORDS]; results[i] = 1 / 0.
 * The host call needs no GPU.  0 / -1. */
int lsr_r1cs_verify_batch(uint32_t m, const uint64_t* public_inputs, size_t n_public, const uint64_t* rows, size_t words_per_row,
                          const uint64_t* proofs, size_t batch, int zk, int* results) LSR_NOEXCEPT;
/* the same on device arrays (the calling thread's current device), asynchronous on `stream`; not capturable (-1) */
int lsr_r1cs_verify_batch_device(uint32_t m, const uint64_t* d_public_inputs, size_t n_public, const uint64_t* d_rows,
                                 size_t words_per_row, const uint64_t* d_proofs, size_t batch, int zk, int* d_results,
                                 void* stream) LSR_NOEXCEPT;
/* eval_poly (r1cs.rs:362-373) over NTT_MODULUS on device arrays: d_values[i][k] = sum_j (c_j mod q) (x mod q)^j mod q with
 * c = d_coeffs[i][0..len), x = d_points[i][k], k < points_per_poly.  Asynchronous on `stream` (current device).  0 / -1. */
int lsr_prover_eval_batch_device(const uint64_t* d_coeffs, size_t len, size_t batch, const uint64_t* d_points,
                                 uint32_t points_per_poly, uint64_t* d_values, void* stream) LSR_NOEXCEPT;

/* ---- the Lagrange (baseline) path: any other circuit (r1cs.rs:596-654, 746-828, 995-1065) ----
 * lsr_r1cs_prover_create_mod builds, for modulus NTT_MODULUS and m a power of two, exactly what lsr_r1cs_prover_create builds;
 * otherwise a Lagrange-path prover for odd 3 <= q < 2^64 and 1 <= m <= 8192.  Its interpolation domain is {omega^j} when
 * q = 17592169062401 and m is in ROOTS_OF_UNITY (4 ... 8192, r1cs.rs:529-575), else {0, 1, ..., m-1}; the quotient always divides
 * by Z_H = prod_{i<m} (X - i) (so on the omega domain a witness with non-zero evaluations leaves a remainder: status 0).  NULL
 * (lsr_last_error says why) for an even q, m outside [1, 8192], a domain whose interpolation denominators are not all units mod q
 * (where the reference panics, e.g. q = 2^44 + 1 with m >= 18), bad shapes, or without a GPU.
 * lsr_r1cs_constraint_evals_batch, lsr_r1cs_quotient_batch and lsr_r1cs_prove_batch[_device] accept either kind with the
 * contracts above (values mod q; the transcript challenges are taken mod q). */
LsrR1csProver* lsr_r1cs_prover_create_mod(const SparseMatrix* A, const SparseMatrix* B, const SparseMatrix* C, uint64_t modulus,
                                          int device) LSR_NOEXCEPT;
uint64_t lsr_r1cs_prover_modulus(const LsrR1csProver* prover) LSR_NOEXCEPT;
/* 1 for a prover on the NTT path, 0 for a Lagrange-path prover */
int      lsr_r1cs_prover_uses_ntt(const LsrR1csProver* prover) LSR_NOEXCEPT;
/* Lagrange-path provers only: a/b/c_coeffs [batch][m] receive the interpolated A_z, B_z, C_z (lagrange_interpolate). 0 / -1. */
int lsr_r1cs_interpolate_batch(LsrR1csProver* prover, const uint64_t* witnesses, size_t batch, uint64_t* a_coeffs, uint64_t* b_coeffs,
                               uint64_t* c_coeffs) LSR_NOEXCEPT;
/* verify_r1cs / verify_r1cs_zk for a circuit with m constraints over `modulus` (odd, >= 3): eval_vanishing is x^m - 1 when
 * modulus = NTT_MODULUS and m is a power of two (then exactly lsr_r1cs_verify_batch), else prod_{i<m} (x - i), m <= 8192.
 * Arguments and results as lsr_r1cs_verify_batch[_device]; the host call needs no GPU.  0 / -1. */
int lsr_r1cs_verify_batch_mod(uint32_t m, uint64_t modulus, const uint64_t* public_inputs, size_t n_public, const uint64_t* rows,
                              size_t words_per_row, const uint64_t* proofs, size_t batch, int zk, int* results) LSR_NOEXCEPT;
int lsr_r1cs_verify_batch_mod_device(uint32_t m, uint64_t modulus, const uint64_t* d_public_inputs, size_t n_public, const uint64_t* d_rows,
                                     size_t words_per_row, const uint64_t* d_proofs, size_t batch, int zk, int* d_results,
                                     void* stream) LSR_NOEXCEPT;

/* ---- the witness-polynomial proofs: prove_simple, prove_zk, simulate_proof and verify_simple (lib.rs:465-491, 551-585, 657-681,
 * 1269-1285; opening.rs:104-115, 160-264; polynomial.rs) ----
 * One proof = LSR_SIMPLE_PROOF_WORDS uint64 words: the challenge alpha, Opening.evaluation and Opening.witness[0] (the commit seed).
 * The commitment is the separate row and Opening.witness[1..] the separate coefficient array coeffs [len] (f' mod q).
 * Moduli: odd 3 <= q < 2^64 (an even q or q < 3: -1 / NULL and lsr_last_error). */
enum { LSR_SIMPLE_ALPHA, LSR_SIMPLE_EVAL, LSR_SIMPLE_SEED, LSR_SIMPLE_PROOF_WORDS };
/* f' = w mod q (prove_simple), f' = (w mod q) + r (prove_zk), f' = r (simulate_proof; no witness), r = random_blinding */
enum { LSR_SIMPLE_PLAIN, LSR_SIMPLE_ZK, LSR_SIMPLE_SIMULATE };
/* ChaCha20Rng::seed_from_u64 (rand_core 0.6.4): keys [count][4] = the 256-bit ChaCha20 keys as little-endian 64-bit words.  Host, no GPU. */
int lsr_chacha20rng_keys_from_u64(const uint64_t* seeds, size_t count, uint64_t* keys) LSR_NOEXCEPT;
/* Polynomial::random_blinding(len - 1, q, .) per key: out[i][j] = (u64 draw j of ChaCha20Rng with key i) mod q, out [batch][len].
 * Host, no GPU.  0 / -1. */
int lsr_random_blinding(const uint64_t* keys, size_t batch, size_t len, uint64_t q, uint64_t* out) LSR_NOEXCEPT;
/* the same on device arrays (the calling thread's current device), asynchronous on `stream`.  0 / -1. */
int lsr_random_blinding_device(const uint64_t* d_keys, size_t batch, size_t len, uint64_t q, uint64_t* d_out, void* stream) LSR_NOEXCEPT;

typedef struct LsrSimpleProver LsrSimpleProver;
/* the Montgomery constants of q and a bounded device workspace on `device` (-1 = default).  NULL for a bad q or without a GPU. */
LsrSimpleProver* lsr_simple_prover_create(uint64_t q, int device) LSR_NOEXCEPT;
void     lsr_simple_prover_free(LsrSimpleProver* prover) LSR_NOEXCEPT;
uint64_t lsr_simple_prover_modulus(const LsrSimpleProver* prover) LSR_NOEXCEPT;
/* `batch` proofs of one length len >= 1 (1 <= len < 2^32).  witnesses [batch][len] (NULL in SIMULATE); public_inputs [batch][n_public]
 * (raw words, hashed as given); seeds [batch] (the commit seeds; 0 = fresh OS entropy for that commitment, as lwe_commit);
 * blinding_keys [batch][4] (ZK / SIMULATE; lsr_chacha20rng_keys_from_u64 of the blinding / sim seeds; NULL = fresh OS entropy per
 * proof, ChaCha20Rng::from_entropy).  Out: rows [batch][lsr_lwe_commitment_words(lwe)] = lwe_commit(f' mod commit_modulus, len, seed)
 * (commit_modulus: Rust's LweContext::modulus()); coeffs [batch][len] = f'; proofs [batch][LSR_SIMPLE_PROOF_WORDS]; hashes
 * [batch][32] (the transcript hash of alpha, may be NULL).  Host arrays, chunked staging.  0 / -1. */
int lsr_simple_prove_batch(LsrSimpleProver* prover, LweContext* lwe, uint64_t commit_modulus, int mode, const uint64_t* witnesses,
                           size_t len, size_t batch, const uint64_t* public_inputs, size_t n_public, const uint64_t* seeds,
                           const uint64_t* blinding_keys, uint64_t* rows, uint64_t* coeffs, uint64_t* proofs, uint8_t* hashes) LSR_NOEXCEPT;
/* the same on device arrays on the prover's device, asynchronous on `stream`.  `seeds` stays a HOST array and every seed must be
 * non-zero; ZK and SIMULATE need d_blinding_keys.  Not capturable into a HIP graph (-1). */
int lsr_simple_prove_batch_device(LsrSimpleProver* prover, LweContext* lwe, uint64_t commit_modulus, int mode, const uint64_t* d_witnesses,
                                  size_t len, size_t batch, const uint64_t* d_public_inputs, size_t n_public, const uint64_t* seeds,
                                  const uint64_t* d_blinding_keys, uint64_t* d_rows, uint64_t* d_coeffs, uint64_t* d_proofs,
                                  uint8_t* d_hashes, void* stream) LSR_NOEXCEPT;
/* verify_simple for `batch` proofs over q: public_inputs [batch][n_public], rows [batch][words_per_row], proofs
 * [batch][LSR_SIMPLE_PROOF_WORDS], coeffs [batch][len] (may be NULL when len = 0); results[i] = 1 / 0.  lwe != NULL adds the binding
 * check of verify_opening_with_context: lwe_verify_opening(lwe, row, (c mod q) mod commit_modulus, len) == 1 (words_per_row must then
 * be lsr_lwe_commitment_words(lwe); a coefficient >= t never opens, as in the reference).  With lwe == NULL the host call needs no
 * GPU.  0 / -1. */
int lsr_simple_verify_batch(uint64_t q, const uint64_t* public_inputs, size_t n_public, const uint64_t* rows, size_t words_per_row,
                            const uint64_t* proofs, const uint64_t* coeffs, size_t len, size_t batch, const LweContext* lwe,
                            uint64_t commit_modulus, int* results) LSR_NOEXCEPT;
/* the same on device arrays (the context's device when lwe != NULL, else the calling thread's current device), asynchronous on
 * `stream` with stream-ordered scratch; not capturable (-1). */
int lsr_simple_verify_batch_device(uint64_t q, const uint64_t* d_public_inputs, size_t n_public, const uint64_t* d_rows,
                                   size_t words_per_row, const uint64_t* d_proofs, const uint64_t* d_coeffs, size_t len, size_t batch,
                                   const LweContext* lwe, uint64_t commit_modulus, int* d_results, void* stream) LSR_NOEXCEPT;

#ifdef __cplusplus
}
#endif
