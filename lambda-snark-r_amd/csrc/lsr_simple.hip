// The witness-polynomial proofs of the reference's lib.rs for a batch: prove_simple, prove_zk, simulate_proof (lib.rs:465-491,
// 551-585, 657-681) and verify_simple (lib.rs:1269-1285), with Polynomial::random_blinding's ChaCha20Rng stream and the optional
// binding check of verify_opening_with_context (opening.rs:160-222).  A prove chunk is: message pass -> commit keys -> commit rows ->
// transcript -> evaluation + record.  Kernels: lsr_simple_kernels.hpp.  C-ABI in lambda_snark/prover.h.
#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "lambda_snark/batch.h"
#include "lambda_snark/prover.h"
#include "lsr_keys.hpp"
#include "lsr_prove_common.hpp"
#include "lsr_runtime.hpp"
#include "lsr_simple_kernels.hpp"

namespace lsr {

// device workspace of one prover: the chunk is sized so that the words below stay within this budget (about 8 k full-length
// instances per chunk on the device path at ring degree 4096, 1.3 k on the host path, which also stages witnesses, rows and
// coefficients)
constexpr size_t kSimpleWorkspaceBytes = size_t(256) << 20;

static unsigned simple_blocks(size_t work, unsigned cap = 256 * 32) {
    return (unsigned)std::max<size_t>(1, std::min<size_t>((work + kSimpleBlock - 1) / kSimpleBlock, cap));
}

static bool odd_modulus(uint64_t q) { return q >= 3 && (q & 1) != 0; }

}  // namespace lsr

struct LsrSimpleProver {
    uint64_t q = 0;
    int device = 0;
    lsr::MontQ M{};
    std::mutex mutex;                       // guards the workspace, the pinned seeds and `stream`; taken before the LWE context's
    lsr::Stream stream;
    lsr::Event ev_last;                     // end of the last asynchronous call: the next call (any stream) starts behind it
    lsr::DeviceBuffer<uint64_t> ws;         // chunk workspace (layout: simple_layout)
    lsr::DeviceBuffer<uint64_t> d_seeds;    // [batch] commit seeds of the current call
    lsr::PinnedBuffer<uint64_t> h_seeds{hipHostMallocDefault};   // their page-locked host copy
};

namespace lsr {

// per chunk of C instances: msg [C][msg_len] | keys [C][4] | bkeys [C][4] | alphas [C] | publics [C][n_public] and, for host
// arrays, witness [C][len] | coeffs [C][len] | rows [C][W] | proofs [C][3] | hashes [C][4]
struct SimpleLayout {
    size_t chunk = 0;
    uint64_t *msg, *keys, *bkeys, *alphas, *publics, *witness, *coeffs, *rows, *proofs, *hashes;
};

static SimpleLayout simple_layout(LsrSimpleProver& p, size_t batch, size_t len, size_t msg_len, size_t n_public, size_t W, bool host_io) {
    const size_t dev = msg_len + 9 + n_public, io = host_io ? 2 * len + W + 7 : 0;
    SimpleLayout L{};
    L.chunk = std::min(batch, std::max<size_t>(1, kSimpleWorkspaceBytes / 8 / (dev + io)));
    const size_t C = L.chunk, words = C * (dev + io);
    p.ws.reserve(words);
    uint64_t* at = p.ws.ptr;
    auto take = [&](size_t n) { uint64_t* r = at; at += n; return r; };
    L.msg = take(C * msg_len);
    L.keys = take(4 * C);
    L.bkeys = take(4 * C);
    L.alphas = take(C);
    L.publics = take(C * n_public);
    if (host_io) {
        L.witness = take(C * len);
        L.coeffs = take(C * len);
        L.rows = take(C * W);
        L.proofs = take(3 * C);
        L.hashes = take(4 * C);
    }
    return L;
}

static void upload_seeds(LsrSimpleProver& p, const uint64_t* seeds, size_t batch, hipStream_t s) {
    p.h_seeds.reserve(batch);
    p.d_seeds.reserve(batch);
    std::memcpy(p.h_seeds.ptr, seeds, batch * 8);
    LSR_HIP(hipMemcpyAsync(p.d_seeds.ptr, p.h_seeds.ptr, batch * 8, hipMemcpyHostToDevice, s));
}

static void launch_message(int mode, const uint64_t* w, const uint64_t* bkeys, uint64_t* coeffs, uint64_t* msg, size_t len, size_t msg_len,
                           uint64_t commit_modulus, size_t count, const MontQ& M, hipStream_t s) {
    const size_t total = count * ((len + 7) / 8);
    const dim3 grid(simple_blocks(total)), block(kSimpleBlock);
    const uint32_t l = (uint32_t)len, ml = (uint32_t)msg_len;
    if (mode == kSimplePlain) hipLaunchKernelGGL(simple_message_kernel<kSimplePlain>, grid, block, 0, s, w, bkeys, coeffs, msg, l, ml, commit_modulus, total, M);
    else if (mode == kSimpleZk) hipLaunchKernelGGL(simple_message_kernel<kSimpleZk>, grid, block, 0, s, w, bkeys, coeffs, msg, l, ml, commit_modulus, total, M);
    else hipLaunchKernelGGL(simple_message_kernel<kSimpleSimulate>, grid, block, 0, s, w, bkeys, coeffs, msg, l, ml, commit_modulus, total, M);
    LSR_HIP(hipGetLastError());
}

static unsigned wave_blocks(size_t count) { return (unsigned)((count + kSimpleBlock / 64 - 1) / (kSimpleBlock / 64)); }

// one chunk: message -> keys -> rows -> alpha -> evaluation + record.  d_* are device arrays of this chunk; seeds / d_seeds its
// commit seeds (host / device); host_keys: derive the commit keys on the host (a seed 0 in the chunk).
struct SimpleChunk {
    const uint64_t *w, *bkeys, *pub, *seeds, *d_seeds;
    uint64_t *coeffs, *rows, *proofs;
    uint8_t* hashes;
    size_t count;
    bool host_keys;
};

static void prove_chunk(LsrSimpleProver& p, LweContext* lwe, uint64_t commit_modulus, int mode, size_t len, size_t msg_len, size_t n_public,
                        const SimpleLayout& L, const SimpleChunk& c, hipStream_t s) {
    const size_t words = lsr_lwe_commitment_words(lwe);
    launch_message(mode, c.w, c.bkeys, c.coeffs, L.msg, len, msg_len, commit_modulus, c.count, p.M, s);
    commit_messages(lwe, L.msg, msg_len, c.count, c.seeds, L.keys, c.rows, c.host_keys, s);
    check_call(lsr_fs_challenge_batch_device(n_public ? c.pub : nullptr, n_public, c.rows, words, c.count, p.q, L.alphas, c.hashes, s),
               "lsr_fs_challenge_batch_device");
    if (len <= kSimpleLaneMaxL)
        hipLaunchKernelGGL(simple_eval_kernel<false>, dim3(simple_blocks(c.count, ~0u)), dim3(kSimpleBlock), 0, s, c.coeffs, (uint32_t)len, L.alphas,
                           c.d_seeds, c.proofs, c.count, p.M);
    else
        hipLaunchKernelGGL(simple_eval_kernel<true>, dim3(wave_blocks(c.count)), dim3(kSimpleBlock), 0, s, c.coeffs, (uint32_t)len, L.alphas, c.d_seeds,
                           c.proofs, c.count, p.M);
    LSR_HIP(hipGetLastError());
}

static size_t msg_len_for(const LweContext* lwe, size_t len) { return std::min<size_t>(len, lsr_lwe_ring_degree(lwe)); }

static void prove_host(LsrSimpleProver& p, LweContext* lwe, uint64_t commit_modulus, int mode, const uint64_t* w, size_t len, size_t batch,
                       const uint64_t* pub, size_t n_public, const uint64_t* seeds, const uint64_t* bkeys, uint64_t* rows, uint64_t* coeffs,
                       uint64_t* proofs, uint8_t* hashes) {
    DeviceGuard guard(p.device);
    std::lock_guard<std::mutex> lock(p.mutex);   // prover first, then (inside each commitment call) the LWE context
    p.ev_last.sync();
    hipStream_t s = p.stream;
    const size_t W = lsr_lwe_commitment_words(lwe), msg_len = msg_len_for(lwe, len);
    std::vector<uint64_t> fresh;                 // ChaCha20Rng::from_entropy for every proof when no keys are given
    if (mode != kSimplePlain && !bkeys) {
        fresh.resize(4 * batch);
        for (size_t i = 0; i < batch; ++i) key_words(fresh_key(), fresh.data() + 4 * i);
        bkeys = fresh.data();
    }
    const SimpleLayout L = simple_layout(p, batch, len, msg_len, n_public, W, true);
    upload_seeds(p, seeds, batch, s);
    for (size_t done = 0; done < batch; done += L.chunk) {
        const size_t now = std::min(L.chunk, batch - done);
        bool zero_seed = false;
        for (size_t j = 0; j < now; ++j) zero_seed |= seeds[done + j] == 0;
        if (mode != kSimpleSimulate) LSR_HIP(hipMemcpyAsync(L.witness, w + done * len, now * len * 8, hipMemcpyHostToDevice, s));
        if (mode != kSimplePlain) LSR_HIP(hipMemcpyAsync(L.bkeys, bkeys + 4 * done, now * 32, hipMemcpyHostToDevice, s));
        if (n_public) LSR_HIP(hipMemcpyAsync(L.publics, pub + done * n_public, now * n_public * 8, hipMemcpyHostToDevice, s));
        const SimpleChunk c{L.witness, L.bkeys, L.publics, seeds + done, p.d_seeds.ptr + done, L.coeffs, L.rows, L.proofs,
                            hashes ? reinterpret_cast<uint8_t*>(L.hashes) : nullptr, now, zero_seed};
        prove_chunk(p, lwe, commit_modulus, mode, len, msg_len, n_public, L, c, s);
        LSR_HIP(hipMemcpyAsync(rows + done * W, L.rows, now * W * 8, hipMemcpyDeviceToHost, s));
        LSR_HIP(hipMemcpyAsync(coeffs + done * len, L.coeffs, now * len * 8, hipMemcpyDeviceToHost, s));
        LSR_HIP(hipMemcpyAsync(proofs + done * 3, L.proofs, now * 24, hipMemcpyDeviceToHost, s));
        if (hashes) LSR_HIP(hipMemcpyAsync(hashes + done * 32, L.hashes, now * 32, hipMemcpyDeviceToHost, s));
        LSR_HIP(hipStreamSynchronize(s));
    }
}

static void prove_device(LsrSimpleProver& p, LweContext* lwe, uint64_t commit_modulus, int mode, const uint64_t* d_w, size_t len, size_t batch,
                         const uint64_t* d_pub, size_t n_public, const uint64_t* seeds, const uint64_t* d_bkeys, uint64_t* d_rows, uint64_t* d_coeffs,
                         uint64_t* d_proofs, uint8_t* d_hashes, hipStream_t s) {
    DeviceGuard guard(p.device);
    std::lock_guard<std::mutex> lock(p.mutex);
    p.ev_last.sync();
    const size_t W = lsr_lwe_commitment_words(lwe), msg_len = msg_len_for(lwe, len);
    const SimpleLayout L = simple_layout(p, batch, len, msg_len, n_public, W, false);
    upload_seeds(p, seeds, batch, s);
    for (size_t done = 0; done < batch; done += L.chunk) {
        const size_t now = std::min(L.chunk, batch - done);
        const SimpleChunk c{d_w ? d_w + done * len : nullptr, d_bkeys ? d_bkeys + 4 * done : nullptr, d_pub ? d_pub + done * n_public : nullptr,
                            seeds + done, p.d_seeds.ptr + done, d_coeffs + done * len, d_rows + done * W, d_proofs + done * 3,
                            d_hashes ? d_hashes + done * 32 : nullptr, now, false};
        prove_chunk(p, lwe, commit_modulus, mode, len, msg_len, n_public, L, c, s);
    }
    p.ev_last.record(s);
}

// ---- verify_simple ---------------------------------------------------------------------------------------------------------------
static void verify_host(uint64_t q, const uint64_t* pub, size_t n_public, const uint64_t* rows, size_t W, const uint64_t* proofs, const uint64_t* coeffs,
                        size_t len, size_t batch, const LweContext* lwe, uint64_t commit_modulus, int* results) {
    std::vector<uint64_t> alphas(batch);
    check_call(lsr_fs_challenge_batch_flat(pub, n_public, rows, W, batch, q, alphas.data(), nullptr, 0), "lsr_fs_challenge_batch_flat");
    const MontQ M = make_mont(q);
    for (size_t i = 0; i < batch; ++i) {
        const uint64_t* p = proofs + 3 * i;
        results[i] = p[0] == alphas[i] && len ? simple_verdict(p, alphas[i], simple_horner<true>(coeffs + i * len, (uint32_t)len, p[0], M), (uint32_t)len, M) : 0;
    }
    if (!lwe) return;
    if (len == 0 || len > lsr_lwe_ring_degree(lwe)) {     // lwe_verify_opening gives 0 or -1 (commitment.cpp:219-221): never 1
        std::fill(results, results + batch, 0);
        return;
    }
    const size_t chunk = std::max<size_t>(1, (size_t(1) << 24) / len);
    std::vector<uint64_t> msg(std::min(batch, chunk) * len);
    std::vector<int> opened(std::min(batch, chunk));
    for (size_t done = 0; done < batch; done += chunk) {
        const size_t now = std::min(chunk, batch - done);
        for (size_t j = 0; j < now * len; ++j) {
            const uint64_t v = mq_canon(coeffs[done * len + j], M);
            msg[j] = v % commit_modulus;
        }
        check_call(lsr_lwe_verify_opening_batch_flat(lwe, rows + done * W, msg.data(), len, now, opened.data()), "lsr_lwe_verify_opening_batch_flat");
        for (size_t j = 0; j < now; ++j) results[done + j] = results[done + j] == 1 && opened[j] == 1 ? 1 : 0;
    }
}

static void verify_device(uint64_t q, const uint64_t* d_pub, size_t n_public, const uint64_t* d_rows, size_t W, const uint64_t* d_proofs,
                          const uint64_t* d_coeffs, size_t len, size_t batch, const LweContext* lwe, uint64_t commit_modulus, int* d_results,
                          hipStream_t s) {
    const MontQ M = make_mont(q);
    const bool open = lwe && len >= 1 && len <= lsr_lwe_ring_degree(lwe);
    const size_t scratch = batch + (open ? batch * len + (batch + 1) / 2 : 0);
    uint64_t* d_scratch = nullptr;
    LSR_HIP(hipMallocAsync(reinterpret_cast<void**>(&d_scratch), scratch * 8, s));
    try {
        uint64_t* alphas = d_scratch;
        check_call(lsr_fs_challenge_batch_device(n_public ? d_pub : nullptr, n_public, d_rows, W, batch, q, alphas, nullptr, s), "lsr_fs_challenge_batch_device");
        if (len <= kSimpleLaneMaxL)
            hipLaunchKernelGGL(simple_check_kernel<false>, dim3(simple_blocks(batch, ~0u)), dim3(kSimpleBlock), 0, s, d_proofs, d_coeffs, (uint32_t)len, alphas,
                               d_results, batch, M);
        else
            hipLaunchKernelGGL(simple_check_kernel<true>, dim3(wave_blocks(batch)), dim3(kSimpleBlock), 0, s, d_proofs, d_coeffs, (uint32_t)len, alphas,
                               d_results, batch, M);
        LSR_HIP(hipGetLastError());
        if (lwe) {
            int* opened = nullptr;
            if (open) {
                uint64_t* msg = d_scratch + batch;
                opened = reinterpret_cast<int*>(msg + batch * len);
                hipLaunchKernelGGL(simple_claim_kernel, dim3(simple_blocks(batch * len)), dim3(kSimpleBlock), 0, s, d_coeffs, msg, commit_modulus, batch * len, M);
                LSR_HIP(hipGetLastError());
                check_call(lsr_lwe_verify_rows_device(lwe, d_rows, msg, len, batch, opened, s), "lsr_lwe_verify_rows_device");
            }
            hipLaunchKernelGGL(simple_and_kernel, dim3(simple_blocks(batch, ~0u)), dim3(kSimpleBlock), 0, s, d_results, opened, batch);
            LSR_HIP(hipGetLastError());
        }
    } catch (...) {
        (void)hipFreeAsync(d_scratch, s);
        throw;
    }
    LSR_HIP(hipFreeAsync(d_scratch, s));
}

// ---- random_blinding ---------------------------------------------------------------------------------------------------------------
// rand_core 0.6.4 SeedableRng::seed_from_u64: eight PCG32 outputs, little endian, fill the 32-byte seed
static void pcg32_key(uint64_t state, uint64_t out[4]) {
    uint32_t w[8];
    for (int i = 0; i < 8; ++i) {
        state = state * 6364136223846793005ull + 11634580027462260723ull;
        const uint32_t xorshifted = (uint32_t)(((state >> 18) ^ state) >> 27);
        const uint32_t rot = (uint32_t)(state >> 59);
        w[i] = (xorshifted >> rot) | (xorshifted << ((32 - rot) & 31));
    }
    for (int i = 0; i < 4; ++i) out[i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
}

static void random_blinding_host(const uint64_t* keys, size_t batch, size_t len, uint64_t q, uint64_t* out) {
    const uint32_t nonce[3] = {0, 0, 0};
    for (size_t i = 0; i < batch; ++i) {
        uint32_t key[8], block[16];
        for (int k = 0; k < 4; ++k) {
            key[2 * k] = (uint32_t)keys[4 * i + k];
            key[2 * k + 1] = (uint32_t)(keys[4 * i + k] >> 32);
        }
        uint64_t* o = out + i * len;
        for (size_t j = 0; j < len; j += 8) {
            chacha20_block_host(key, (uint32_t)(j / 8), nonce, block);
            for (size_t t = 0; t < 8 && j + t < len; ++t) o[j + t] = (((uint64_t)block[2 * t + 1] << 32) | block[2 * t]) % q;
        }
    }
}

}  // namespace lsr

using lsr::abi_guarded;
using lsr::abi_refuse;

static void destroy_simple(LsrSimpleProver* p) {
    if (!p) return;
    try {
        lsr::DeviceGuard guard(p->device);
        p->ev_last.sync();
        delete p;
    } catch (...) {
        delete p;
    }
}

static int prove_args(const char* where, const LsrSimpleProver* p, const LweContext* lwe, uint64_t commit_modulus, int mode, const void* w, size_t len,
                      size_t batch, const void* pub, size_t n_public, const void* seeds, const void* rows, const void* coeffs, const void* proofs) {
    if (!p || !lwe) return abi_refuse(where, "NULL prover or LWE context");
    if (mode != LSR_SIMPLE_PLAIN && mode != LSR_SIMPLE_ZK && mode != LSR_SIMPLE_SIMULATE) return abi_refuse(where, "unknown mode");
    if (len == 0) return abi_refuse(where, "Witness cannot be empty (len must be >= 1)");
    if (len > 0xffffffffull) return abi_refuse(where, "len must be below 2^32");
    if (batch == 0) return 0;
    if ((mode != LSR_SIMPLE_SIMULATE && !w) || (!pub && n_public) || !seeds || !rows || !coeffs || !proofs)
        return abi_refuse(where, "NULL witnesses, public inputs, seeds or output");
    if (commit_modulus <= 1) return abi_refuse(where, "commit_modulus must be LweContext::modulus() (> 1)");
    if (lsr::refuse_rns_context(where, lwe)) return -1;
    const NttContext* ntt = lsr_lwe_ntt_context(lwe);
    if (!ntt || ntt->device != p->device) return abi_refuse(where, "the prover and the LWE context live on different devices");
    return 0;
}

static int verify_args(const char* where, uint64_t q, const void* pub, size_t n_public, const void* rows, size_t words, const void* proofs,
                       const void* coeffs, size_t len, const LweContext* lwe, uint64_t commit_modulus, const void* results) {
    if (!lsr::odd_modulus(q)) return abi_refuse(where, "the modulus must be odd and >= 3");
    if ((!pub && n_public) || !rows || !proofs || (!coeffs && len) || !results) return abi_refuse(where, "NULL public inputs, rows, proofs, coefficients or results");
    if (words == 0) return abi_refuse(where, "words_per_row must be positive");
    if (len > 0xffffffffull) return abi_refuse(where, "len must be below 2^32");
    if (lwe) {
        if (commit_modulus <= 1) return abi_refuse(where, "commit_modulus must be LweContext::modulus() (> 1)");
        if (lsr::refuse_rns_context(where, lwe)) return -1;
        if (words != lsr_lwe_commitment_words(lwe)) return abi_refuse(where, "words_per_row must be the context's commitment words");
    }
    return 0;
}

extern "C" {

int lsr_chacha20rng_keys_from_u64(const uint64_t* seeds, size_t count, uint64_t* keys) noexcept {
    if (count && (!seeds || !keys)) return abi_refuse("lsr_chacha20rng_keys_from_u64", "NULL seeds or keys");
    for (size_t i = 0; i < count; ++i) lsr::pcg32_key(seeds[i], keys + 4 * i);
    return 0;
}

int lsr_random_blinding(const uint64_t* keys, size_t batch, size_t len, uint64_t q, uint64_t* out) noexcept {
    const char* where = "lsr_random_blinding";
    if (!lsr::odd_modulus(q)) return abi_refuse(where, "the modulus must be odd and >= 3");
    if (batch && len && (!keys || !out)) return abi_refuse(where, "NULL keys or output");
    if (len > 0xffffffffull) return abi_refuse(where, "len must be below 2^32");
    return abi_guarded(where, [&] { lsr::random_blinding_host(keys, batch, len, q, out); });
}

int lsr_random_blinding_device(const uint64_t* d_keys, size_t batch, size_t len, uint64_t q, uint64_t* d_out, void* stream) noexcept {
    const char* where = "lsr_random_blinding_device";
    if (!lsr::odd_modulus(q)) return abi_refuse(where, "the modulus must be odd and >= 3");
    if (batch && len && (!d_keys || !d_out)) return abi_refuse(where, "NULL keys or output");
    if (len > 0xffffffffull) return abi_refuse(where, "len must be below 2^32");
    if (batch == 0 || len == 0) return 0;
    return abi_guarded(where, [&] {
        lsr::launch_message(lsr::kSimpleSimulate, nullptr, d_keys, d_out, nullptr, len, 0, 1, batch, lsr::make_mont(q), static_cast<hipStream_t>(stream));
    });
}

LsrSimpleProver* lsr_simple_prover_create(uint64_t q, int device) noexcept {
    const char* where = "lsr_simple_prover_create";
    if (!lsr::odd_modulus(q)) {
        abi_refuse(where, "the modulus must be odd and >= 3");
        return nullptr;
    }
    device = lsr::resolve_device(where, device, false);
    if (device < 0) return nullptr;
    try {
        std::unique_ptr<LsrSimpleProver, lsr::HandleDeleter<LsrSimpleProver, destroy_simple>> p(new LsrSimpleProver);
        p->q = q;
        p->device = device;
        p->M = lsr::make_mont(q);
        lsr::DeviceGuard guard(device);
        LSR_HIP(hipStreamCreateWithFlags(&p->stream.handle, hipStreamNonBlocking));
        return p.release();
    } catch (const std::exception& e) {
        abi_refuse(where, e.what());
        return nullptr;
    }
}

void lsr_simple_prover_free(LsrSimpleProver* prover) noexcept { destroy_simple(prover); }
uint64_t lsr_simple_prover_modulus(const LsrSimpleProver* prover) noexcept { return prover ? prover->q : 0; }

int lsr_simple_prove_batch(LsrSimpleProver* prover, LweContext* lwe, uint64_t commit_modulus, int mode, const uint64_t* witnesses, size_t len,
                           size_t batch, const uint64_t* public_inputs, size_t n_public, const uint64_t* seeds, const uint64_t* blinding_keys,
                           uint64_t* rows, uint64_t* coeffs, uint64_t* proofs, uint8_t* hashes) noexcept {
    const char* where = "lsr_simple_prove_batch";
    if (prove_args(where, prover, lwe, commit_modulus, mode, witnesses, len, batch, public_inputs, n_public, seeds, rows, coeffs, proofs)) return -1;
    if (batch == 0) return 0;
    return abi_guarded(where, [&] {
        lsr::prove_host(*prover, lwe, commit_modulus, mode, witnesses, len, batch, public_inputs, n_public, seeds, blinding_keys, rows, coeffs, proofs,
                        hashes);
    });
}

int lsr_simple_prove_batch_device(LsrSimpleProver* prover, LweContext* lwe, uint64_t commit_modulus, int mode, const uint64_t* d_witnesses, size_t len,
                                  size_t batch, const uint64_t* d_public_inputs, size_t n_public, const uint64_t* seeds, const uint64_t* d_blinding_keys,
                                  uint64_t* d_rows, uint64_t* d_coeffs, uint64_t* d_proofs, uint8_t* d_hashes, void* stream) noexcept {
    const char* where = "lsr_simple_prove_batch_device";
    if (prove_args(where, prover, lwe, commit_modulus, mode, d_witnesses, len, batch, d_public_inputs, n_public, seeds, d_rows, d_coeffs, d_proofs)) return -1;
    if (batch == 0) return 0;
    if (mode != LSR_SIMPLE_PLAIN && !d_blinding_keys) return abi_refuse(where, "ZK and SIMULATE need device blinding keys (fresh entropy is the host call's)");
    return lsr::abi_prove_device(where, "lsr_simple_prove_batch", seeds, batch, prover->device, stream, [&](hipStream_t s) {
        lsr::prove_device(*prover, lwe, commit_modulus, mode, d_witnesses, len, batch, d_public_inputs, n_public, seeds, d_blinding_keys, d_rows, d_coeffs,
                          d_proofs, d_hashes, s);
    });
}

int lsr_simple_verify_batch(uint64_t q, const uint64_t* public_inputs, size_t n_public, const uint64_t* rows, size_t words_per_row, const uint64_t* proofs,
                            const uint64_t* coeffs, size_t len, size_t batch, const LweContext* lwe, uint64_t commit_modulus, int* results) noexcept {
    const char* where = "lsr_simple_verify_batch";
    if (verify_args(where, q, public_inputs, n_public, rows, words_per_row, proofs, coeffs, len, lwe, commit_modulus, results)) return -1;
    if (batch == 0) return 0;
    return abi_guarded(where, [&] {
        lsr::verify_host(q, public_inputs, n_public, rows, words_per_row, proofs, coeffs, len, batch, lwe, commit_modulus, results);
    });
}

int lsr_simple_verify_batch_device(uint64_t q, const uint64_t* d_public_inputs, size_t n_public, const uint64_t* d_rows, size_t words_per_row,
                                   const uint64_t* d_proofs, const uint64_t* d_coeffs, size_t len, size_t batch, const LweContext* lwe,
                                   uint64_t commit_modulus, int* d_results, void* stream) noexcept {
    const char* where = "lsr_simple_verify_batch_device";
    if (verify_args(where, q, d_public_inputs, n_public, d_rows, words_per_row, d_proofs, d_coeffs, len, lwe, commit_modulus, d_results)) return -1;
    if (batch == 0) return 0;
    if (batch > 0x7fffffffull) return abi_refuse(where, "batch exceeds 2^31 - 1 proofs");
    return abi_guarded(where, [&] {
        const NttContext* ntt = lwe ? lsr_lwe_ntt_context(lwe) : nullptr;
        if (lwe && !ntt) throw std::runtime_error("the LWE context has no device");
        int device = 0;
        LSR_HIP(hipGetDevice(&device));
        lsr::DeviceGuard guard(ntt ? ntt->device : device);
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (lsr::stream_is_capturing(s)) throw std::runtime_error("not capturable into a HIP graph (stream-ordered scratch)");
        lsr::verify_device(q, d_public_inputs, n_public, d_rows, words_per_row, d_proofs, d_coeffs, len, batch, lwe, commit_modulus, d_results, s);
    });
}

}  // extern "C"
