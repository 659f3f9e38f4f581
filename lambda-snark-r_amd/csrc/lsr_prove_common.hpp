// Host pipeline shared by the prover paths: the NTT path (lsr_prover.hip), the Lagrange path (lsr_lagrange.hip) and the simple
// proofs (lsr_simple.hip).  The kernels stay with their paths; this holds the steps around them — the commitment step, the R1CS
// transcript, scratch layout, chunk drivers and verifier — and the refusals of the batched device entry points.
#pragma once

#include <algorithm>
#include <mutex>
#include <vector>

#include "lambda_snark/batch.h"
#include "lambda_snark/r1cs.h"
#include "lsr_runtime.hpp"

namespace lsr {

// an ABI return code of a commitment or transcript entry point, as an exception
inline void check_call(int rc, const char* what) {
    if (rc != 0) throw std::runtime_error(std::string(what) + ": " + lsr_last_error());
}

// The provers and their verifiers commit and open under ONE modulus: a two-prime RNS context (batch.h, lsr_lwe_context_create_rns)
// is refused by their argument checks.  `lwe` non-NULL.
inline int refuse_rns_context(const char* where, const LweContext* lwe) {
    uint64_t moduli[2];
    if (lsr_lwe_rns_moduli(lwe, moduli) != 0) return 0;
    return abi_refuse(where, "RNS contexts (lsr_lwe_context_create_rns) are not supported by the provers and their verifiers");
}

// keys and rows of `count` commitments to the device messages d_msg [count][msg_len], all on `s`.  host_keys: derive the keys on
// the host (seed 0 = fresh entropy) from the messages copied back; else on the device.
inline void commit_messages(LweContext* lwe, const uint64_t* d_msg, size_t msg_len, size_t count, const uint64_t* seeds, uint64_t* d_keys,
                            uint64_t* d_rows, bool host_keys, hipStream_t s) {
    if (host_keys) {
        std::vector<uint64_t> msgs(count * msg_len), keys(4 * count);
        LSR_HIP(hipMemcpyAsync(msgs.data(), d_msg, msgs.size() * 8, hipMemcpyDeviceToHost, s));
        LSR_HIP(hipStreamSynchronize(s));
        check_call(lsr_lwe_commit_keys(lwe, msgs.data(), msg_len, count, seeds, keys.data()), "lsr_lwe_commit_keys");
        LSR_HIP(hipMemcpyAsync(d_keys, keys.data(), keys.size() * 8, hipMemcpyHostToDevice, s));
        LSR_HIP(hipStreamSynchronize(s));   // `keys` leaves scope
    } else {
        check_call(lsr_lwe_commit_keys_device(lwe, d_msg, msg_len, count, seeds, d_keys, s), "lsr_lwe_commit_keys_device");
    }
    check_call(lsr_lwe_commit_rows_device(lwe, d_msg, msg_len, count, d_keys, d_rows, s), "lsr_lwe_commit_rows_device");
}

// The entry of a batched prove call on the device: refuses a seed 0 (fresh OS entropy, which only the host call `host_call` serves)
// and a batch beyond 2^31 - 1, then runs body(stream) on `device` unless the stream is being captured into a HIP graph.
template <class F>
int abi_prove_device(const char* where, const char* host_call, const uint64_t* seeds, size_t batch, int device, void* stream, F&& body) noexcept {
    for (size_t i = 0; i < batch; ++i)
        if (seeds[i] == 0)
            return abi_refuse(where, std::string("seed 0 asks for fresh OS entropy, which only the host call serves (") + host_call + ")");
    if (batch > 0x7fffffffull) return abi_refuse(where, "batch exceeds 2^31 - 1 proofs");
    return abi_guarded(where, [&] {
        DeviceGuard guard(device);
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (stream_is_capturing(s)) throw std::runtime_error("not capturable into a HIP graph (host seeds, host-ordered workspace)");
        body(s);
    });
}

// ---- the R1CS matrices of a prover, both R1CS paths ---------------------------------------------------------------------------------

// A, B, C share one m x n_vars shape, n_vars > 0, and every entry lies inside it; else false and lsr_last_error "<where>: <why>"
inline bool r1cs_shape_ok(const char* where, const SparseMatrix* const mats[3]) {
    const uint32_t m = mats[0]->n_rows, n_vars = mats[0]->n_cols;
    for (int k = 0; k < 3; ++k) {
        if (mats[k]->n_rows != m || mats[k]->n_cols != n_vars || (mats[k]->n_entries && !mats[k]->entries) || mats[k]->n_entries > 0xFFFFFFF0ull) {
            set_last_error(std::string(where) + ": A, B, C must share one shape");
            return false;
        }
        for (size_t e = 0; e < mats[k]->n_entries; ++e)
            if (mats[k]->entries[e].row >= m || mats[k]->entries[e].col >= n_vars) {
                set_last_error(std::string(where) + ": entry outside the matrix");
                return false;
            }
    }
    if (n_vars == 0) {
        set_last_error(std::string(where) + ": no variables");
        return false;
    }
    return true;
}

// the coordinate form of checked matrices -> CSR on the device (stable counting sort by row); value(v) is an entry's value in the path's form
template <class Value>
void upload_csr(const SparseMatrix* const mats[3], DeviceBuffer<uint32_t> (&row_ptr)[3], DeviceBuffer<uint32_t> (&col)[3], DeviceBuffer<uint64_t> (&val)[3],
                Value&& value) {
    const uint32_t m = mats[0]->n_rows;
    for (int k = 0; k < 3; ++k) {
        const SparseMatrix& M = *mats[k];
        std::vector<uint32_t> ptr(m + 1, 0), cols(M.n_entries);
        std::vector<uint64_t> vals(M.n_entries);
        for (size_t e = 0; e < M.n_entries; ++e) ++ptr[M.entries[e].row + 1];
        for (uint32_t i = 0; i < m; ++i) ptr[i + 1] += ptr[i];
        std::vector<uint32_t> cursor(ptr.begin(), ptr.end() - 1);
        for (size_t e = 0; e < M.n_entries; ++e) {
            const uint32_t at = cursor[M.entries[e].row]++;
            cols[at] = M.entries[e].col;
            vals[at] = value(M.entries[e].value);
        }
        row_ptr[k].upload(ptr);
        if (M.n_entries == 0) { cols.push_back(0); vals.push_back(0); }   // keep the pointers non-null
        col[k].upload(cols);
        val[k].upload(vals);
    }
}

// ---- prove_r1cs / prove_r1cs_zk (lib.rs:747-809, 877-980), both R1CS paths ---------------------------------------------------------

struct R1csSlots {             // one chunk's views into the per-instance scratch
    uint64_t *keys, *alphas, *betas, *hash_a, *hash_b, *ev, *blinding, *publics;
};

// The per-instance scratch of an R1CS prover and its host staging.  chunk, publics and row_words describe the layout of the buffers:
// each is committed only once the buffers laid out by it are allocated, and every gate reads the buffers' own counts.
struct R1csScratch {
    size_t chunk = 0, publics = 0, row_words = 0;
    DeviceBuffer<uint64_t> small;      // keys[4] alphas betas hash_a[4] hash_b[4] ev[8] blinding publics[n_public] per instance
    DeviceBuffer<uint64_t> io;         // host staging: rows [chunk][row_words] then proofs [chunk][13] then hashes [chunk][8]
    DeviceBuffer<uint32_t> io_status;  // [chunk]

    R1csSlots slots() const {
        uint64_t* b = small.ptr;
        R1csSlots v;
        v.keys = b;                 b += 4 * chunk;
        v.alphas = b;               b += chunk;
        v.betas = b;                b += chunk;
        v.hash_a = b;               b += 4 * chunk;
        v.hash_b = b;               b += 4 * chunk;
        v.ev = b;                   b += 8 * chunk;
        v.blinding = b;             b += chunk;
        v.publics = b;
        return v;
    }
    // sizes the scratch for at least `want` instances and `n_public` publics (grows only; the staging is then dropped).  A path first
    // reserves its own chunk-sized buffers for max(chunk, want) instances, then calls this.
    void grow(size_t want, size_t n_public) {
        const size_t c = std::max(chunk, want), pub = std::max(publics, n_public);
        const size_t words = c * (23 + std::max<size_t>(1, pub));
        if (small.count >= words) return;
        io.release();
        io_status.release();
        row_words = 0;
        small.allocate(words);
        chunk = c;
        publics = pub;
    }
    // the host staging, for rows of `words` words
    void stage(size_t words) {
        const size_t rw = std::max<size_t>({row_words, words, 1});
        if (io.count >= chunk * (rw + 13 + 8) && io_status.count >= chunk) return;
        io.allocate(chunk * (rw + 13 + 8));
        io_status.allocate(chunk);
        row_words = rw;
    }
};

// alpha = Challenge::derive(public_inputs, row), beta = Challenge::derive([alpha], row) (lib.rs:761-768) of `count` instances, with the
// hash outputs, all on `s`.  `gather` is the path's kernel that copies the n_public leading words of each witness d_z [count][n_vars].
using GatherPublicsKernel = void (*)(const uint64_t*, uint32_t, uint32_t, uint64_t*, size_t);
inline void r1cs_transcript(GatherPublicsKernel gather, const R1csSlots& v, const uint64_t* d_z, uint32_t n_vars, size_t n_public, const uint64_t* d_rows,
                            size_t words, size_t count, uint64_t q, hipStream_t s) {
    if (n_public) {
        const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>((count * n_public + 255) / 256, 256 * 32));
        hipLaunchKernelGGL(gather, dim3(grid), dim3(256), 0, s, d_z, n_vars, (uint32_t)n_public, v.publics, count * n_public);
    }
    LSR_HIP(hipGetLastError());
    check_call(lsr_fs_challenge_chain_batch_device(LSR_FS_PATH_AUTO, n_public ? v.publics : nullptr, n_public, d_rows, words, count, q, v.alphas, v.betas,
                                                   reinterpret_cast<uint8_t*>(v.hash_a), reinterpret_cast<uint8_t*>(v.hash_b), s),
               "lsr_fs_challenge_chain_batch_device");
}

// One batched call: host arrays (r1cs_prove_host) or device arrays (r1cs_prove_device); `seeds` is a host array either way.
struct R1csProveCall {
    LweContext* lwe;
    uint64_t commit_modulus;
    size_t n_public;
    const uint64_t* seeds;     // [batch]
    const uint64_t* w;         // witnesses [batch][n_vars]
    const uint64_t* blind;     // [batch] (prove_r1cs_zk) or nullptr
    uint64_t* rows;            // [batch][lsr_lwe_commitment_words(lwe)]
    uint64_t* proofs;          // [batch][13]
    uint8_t* hashes;           // [batch][64] or nullptr
    uint32_t* status;          // [batch]
    size_t batch;
};

// What a path lends the drivers.  Its mutex is taken first, then (inside each commitment call) the LWE context's; ev_last marks the
// end of its last asynchronous call.
struct R1csProverRef {
    int device;
    std::mutex& mutex;
    Event& ev_last;
    hipStream_t stream;                  // the path's own stream: host calls
    DeviceBuffer<uint64_t>& witness;     // [chunk][n_vars]: host calls
    uint32_t n_vars;
    R1csScratch& ws;
};

// The drivers take the path's chunk size, grow(chunk) that sizes its workspace and the scratch, and
// prove_chunk(d_z, d_blind, seeds, count, d_rows, d_proofs, d_hashes, d_status, host_keys, s) that proves `count` instances on `s`.
template <class Grow, class ProveChunk>
void r1cs_prove_host(const R1csProverRef& r, const R1csProveCall& c, size_t chunk, Grow&& grow, ProveChunk&& prove_chunk) {
    DeviceGuard guard(r.device);
    std::lock_guard<std::mutex> lock(r.mutex);
    r.ev_last.sync();
    const size_t words = lsr_lwe_commitment_words(c.lwe);
    grow(chunk);
    r.ws.stage(words);
    hipStream_t s = r.stream;
    uint64_t* d_blind = r.ws.slots().blinding;
    uint64_t* d_rows = r.ws.io.ptr;
    uint64_t* d_proofs = d_rows + r.ws.chunk * r.ws.row_words;
    uint64_t* d_hashes = d_proofs + r.ws.chunk * 13;
    for (size_t done = 0; done < c.batch; done += chunk) {
        const size_t now = std::min(chunk, c.batch - done);
        bool zero_seed = false;
        for (size_t j = 0; j < now; ++j) zero_seed |= c.seeds[done + j] == 0;
        LSR_HIP(hipMemcpyAsync(r.witness.ptr, c.w + done * r.n_vars, now * r.n_vars * 8, hipMemcpyHostToDevice, s));
        if (c.blind) LSR_HIP(hipMemcpyAsync(d_blind, c.blind + done, now * 8, hipMemcpyHostToDevice, s));
        prove_chunk(r.witness.ptr, c.blind ? d_blind : nullptr, c.seeds + done, now, d_rows, d_proofs, c.hashes ? reinterpret_cast<uint8_t*>(d_hashes) : nullptr,
                    r.ws.io_status.ptr, zero_seed, s);
        LSR_HIP(hipMemcpyAsync(c.rows + done * words, d_rows, now * words * 8, hipMemcpyDeviceToHost, s));
        LSR_HIP(hipMemcpyAsync(c.proofs + done * 13, d_proofs, now * 13 * 8, hipMemcpyDeviceToHost, s));
        if (c.hashes) LSR_HIP(hipMemcpyAsync(c.hashes + done * 64, d_hashes, now * 64, hipMemcpyDeviceToHost, s));
        LSR_HIP(hipMemcpyAsync(c.status + done, r.ws.io_status.ptr, now * 4, hipMemcpyDeviceToHost, s));
        LSR_HIP(hipStreamSynchronize(s));
    }
}

template <class Grow, class ProveChunk>
void r1cs_prove_device(const R1csProverRef& r, const R1csProveCall& c, size_t chunk, Grow&& grow, ProveChunk&& prove_chunk, hipStream_t s) {
    DeviceGuard guard(r.device);
    std::lock_guard<std::mutex> lock(r.mutex);
    r.ev_last.sync();
    const size_t words = lsr_lwe_commitment_words(c.lwe);
    grow(chunk);
    for (size_t done = 0; done < c.batch; done += chunk) {
        const size_t now = std::min(chunk, c.batch - done);
        prove_chunk(c.w + done * r.n_vars, c.blind ? c.blind + done : nullptr, c.seeds + done, now, c.rows + done * words, c.proofs + done * 13,
                    c.hashes ? c.hashes + done * 64 : nullptr, c.status + done, false, s);
    }
    r.ev_last.record(s);
}

// ---- verify_r1cs / verify_r1cs_zk, both R1CS paths: the two transcripts, then the path's per-proof check -----------------------------

// on the host (transcripts on the host pool, lsr_fs_challenge_chain_batch_flat): results[i] = check(proof i, alpha_i, beta_i)
template <class Check>
void r1cs_verify_host(uint64_t q, const uint64_t* pub, size_t n_public, const uint64_t* rows, size_t words, const uint64_t* proofs, size_t batch,
                      int* results, Check&& check) {
    std::vector<uint64_t> alphas(batch), betas(batch);
    check_call(lsr_fs_challenge_chain_batch_flat(pub, n_public, rows, words, batch, q, alphas.data(), betas.data(), nullptr, nullptr, 0),
               "lsr_fs_challenge_chain_batch_flat");
    for (size_t i = 0; i < batch; ++i) results[i] = check(proofs + i * 13, alphas[i], betas[i]);
}

// on the device, all on `s`: alphas and betas in stream-ordered scratch, then launch_check(d_alphas, d_betas) enqueues the check kernel
template <class LaunchCheck>
void r1cs_verify_device(uint64_t q, const uint64_t* d_pub, size_t n_public, const uint64_t* d_rows, size_t words, size_t batch, hipStream_t s,
                        LaunchCheck&& launch_check) {
    if (stream_is_capturing(s)) throw std::runtime_error("not capturable into a HIP graph (stream-ordered scratch)");
    uint64_t* d_ab = nullptr;
    LSR_HIP(hipMallocAsync(reinterpret_cast<void**>(&d_ab), 2 * batch * 8, s));
    try {
        check_call(lsr_fs_challenge_chain_batch_device(LSR_FS_PATH_AUTO, d_pub, n_public, d_rows, words, batch, q, d_ab, d_ab + batch, nullptr, nullptr, s),
                   "lsr_fs_challenge_chain_batch_device");
        launch_check(d_ab, d_ab + batch);
        LSR_HIP(hipGetLastError());
    } catch (...) {
        (void)hipFreeAsync(d_ab, s);
        throw;
    }
    LSR_HIP(hipFreeAsync(d_ab, s));
}

}  // namespace lsr
