// The ring handle under an arbitrary modulus (LsrRingMod, batch.h) as the translation units that read it see it:
// lsr_ring_mod.hip creates it, computes mul, dot and dot_galois and lends its coefficient context (§5t), lsr_ring_mod_matvec.hip keeps
// resident matrices on it (§5q), lsr_ring_mod_gram.hip computes Gram matrices of bounded vectors on it (§5r), lsr_ring_mod_fold.hip folds vectors by challenges on it (§5s),
// lsr_ring_mod_quadform.hip evaluates quadratic forms of a packed Gram triangle on it (§5u).  The call path they share — the bracket
// of a call, the views of the two workspaces, the checked lift and the gated reduce — is lsr_ring_mod_call.hpp.
#pragma once

#include <mutex>

#include "lsr_ring_mod_kernels.hpp"
#include "lsr_runtime.hpp"

struct LsrRingMod {
    // q and n stay the first fields: lsr_ring_mod_modulus reads nothing but q, and the refusals that precede device work read nothing else
    uint64_t q = 0;
    uint32_t n = 0;
    int logn = 0;
    int device = 0;
    size_t max_terms = 0;
    lsr::NttContextPtr prime[2];
    lsr::NttContextPtr coeff;        // (q, n) without tables: lent out by lsr_ring_mod_coeff_context
    lsr::RingModConsts rc{};
    lsr::ModParams pq{};             // of q: only q and floor(2^128 / q) are used
    lsr::LiftSource lift[2]{};
    // n <= 4096: [2][chunk][n] inverse-transformed sums, then [2][bhat_rows][n] transforms of a shared b or of a fold's challenges, then
    // kRingModFoldFlagWords words of flags, a fold's per output or a bounded matrix product's per vector (ring_mod_workspace,
    // lsr_ring_mod_call.hpp).  Never resized.
    size_t chunk = 0, bhat_rows = 0;
    lsr::DeviceBuffer<uint64_t> ws;
    // the Gram calls and the quadratic forms (lsr_ring_mod_gram.hip, lsr_ring_mod_quadform.hip): [2][ring_mod_gram_words()] lifted operands, their transforms and the outputs of one chunk
    // per prime, then kRingModGramFlagWords words of per-family flags.  Allocated by the first eager Gram call or by
    // lsr_ring_mod_gram_prepare under `mutex`, never resized.
    mutable lsr::DeviceBuffer<uint64_t> gram_ws;
    // calls on one handle are ordered like the ring calls of a context (lsr_ring_mod_call.hpp ring_mod_call)
    mutable std::mutex mutex;
    mutable lsr::Event event;
};

namespace lsr {

constexpr size_t kRingModSumWords = (size_t)1 << 22;    // per prime: 32 MiB, both arrays stay in the Infinity Cache for the reduce
constexpr size_t kRingModBhatWords = (size_t)1 << 21;   // per prime
constexpr size_t kRingModBhatMaxRows = 4096;            // bhat_rows = min(this, kRingModBhatWords / n)
constexpr size_t kRingModFoldFlagWords = kRingModBhatMaxRows / 2;   // 32-bit flag words: one per challenge row

// Gram workspace words per prime: a function of the process-wide chunk size alone (a quarter of it, 64 MiB of 256: the two halves stay in
// the Infinity Cache between the passes of a chunk), at least 2^23 words
size_t ring_mod_gram_words();
constexpr size_t kRingModGramFlagWords = (size_t)1 << 15;   // 65536 32-bit flag words: the families of one chunk are one grid axis

// the two streaming kernels on `s` (lsr_ring_mod.hip): no workspace, no ordering
void launch_lift(const LsrRingMod& h, int i, uint64_t* d_out, const uint64_t* d_x, size_t count, hipStream_t s);
void launch_reduce(const LsrRingMod& h, uint64_t* d_out, const uint64_t* d_r0, const uint64_t* d_r1, size_t count, bool accumulate, hipStream_t s);

// `count` UNIFORM elements of Z_q[X]/(X^n + 1), n = 2^logn, as lsr_ntt_ring_sample_batch defines them with modulus q, one key (four
// words on the device) and stream indices index_base + e (lsr_ring_sample.hip); enqueues kernels on `s` and nothing else
void sample_uniform_device(uint64_t q, int logn, uint64_t* d_out, uint64_t count, const uint64_t* d_key, uint32_t domain, uint64_t index_base,
                           hipStream_t s);

}  // namespace lsr
