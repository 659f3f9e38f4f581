// Host interface of the Lagrange (baseline) prove path, lsr_lagrange.hip.  lsr_prover.hip dispatches the
// prover.h entry points here when an LsrR1csProver was built by lsr_r1cs_prover_create_mod off the NTT path.
#pragma once

#include <cstddef>
#include <cstdint>

#include "lambda_snark/r1cs.h"
#include "lambda_snark/types.h"
#include "lsr_prove_common.hpp"

namespace lsr {

struct LagrangeProver;

constexpr uint32_t kLagrangeMaxM = 8192;
constexpr uint64_t kQuirkModulus = 17592169062401ull;   // NTT_FRIENDLY_MODULUS, r1cs.rs:529

// nullptr (+ lsr_last_error) on bad shapes, an even q or q < 3, m outside [1, 8192], a non-unit interpolation denominator, or no GPU
LagrangeProver* lagrange_create(const SparseMatrix* const mats[3], uint64_t q, int device);
void lagrange_destroy(LagrangeProver* p);
using LagrangeProverPtr = std::unique_ptr<LagrangeProver, HandleDeleter<LagrangeProver, lagrange_destroy>>;
int lagrange_device(const LagrangeProver* p);
bool lagrange_omega_domain(const LagrangeProver* p);

// host arrays.  evals != nullptr: A z, B z, C z; coeffs != nullptr: the interpolated A, B, C; else quotient / len.  Throws.
void lagrange_host_run(LagrangeProver& p, const uint64_t* w, size_t batch, uint64_t* const evals[3], uint64_t* const coeffs[3], uint64_t* quotient,
                       uint32_t* len);
// prove_r1cs[_zk] for a batch: device arrays on `s` (on_device) or host arrays through the prover's own stream.  Throws.
void lagrange_prove(LagrangeProver& p, const R1csProveCall& c, bool on_device, hipStream_t s);

// verify_r1cs[_zk] on the baseline path (eval_vanishing = prod (x - i)) for modulus q
void verify_mod_host(uint32_t m, uint64_t q, const uint64_t* pub, size_t n_public, const uint64_t* rows, size_t words, const uint64_t* proofs,
                     size_t batch, bool zk, int* results);
void verify_mod_device(uint32_t m, uint64_t q, const uint64_t* d_pub, size_t n_public, const uint64_t* d_rows, size_t words, const uint64_t* d_proofs,
                       size_t batch, bool zk, int* d_results, hipStream_t s);

}  // namespace lsr
