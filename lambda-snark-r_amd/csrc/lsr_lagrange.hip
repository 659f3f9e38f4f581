// The Lagrange (baseline) path of compute_quotient_poly / prove_r1cs / verify_r1cs for any odd modulus q < 2^64 and
// 1 <= m <= 8192 constraints (rust-api/lambda-snark/src/r1cs.rs:596-654, 746-828, 995-1065; lib.rs:747-980, 1016-1215).
// The plan holds the interpolation matrix L of its domain, the power series of 1 / rev(Z_H) and Z_H itself; a batch of
// witnesses then costs one modular GEMM plus O(m^2) work per instance.  Kernels: lsr_lagrange_kernels.hpp.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "lambda_snark/batch.h"
#include "lambda_snark/prover.h"
#include "lsr_lagrange.hpp"
#include "lsr_lagrange_kernels.hpp"
#include "lsr_prove_common.hpp"
#include "lsr_runtime.hpp"

namespace lsr {

// ROOTS_OF_UNITY of r1cs.rs:533-547: the omega domain of NTT_FRIENDLY_MODULUS (get_ntt_root, r1cs.rs:563-575)
static const struct { uint32_t m; uint64_t omega; } kQuirkRoots[] = {
    {4, 981206394875ull},       {8, 4268641988953ull},      {16, 9400386778549ull},    {32, 15690227524213ull},
    {64, 8332322609789ull},     {128, 9249819209096ull},    {256, 5221410271124ull},   {512, 9594533594163ull},
    {1024, 11016271016603ull},  {2048, 14373677444369ull},  {4096, 11176258803537ull}, {8192, 9037003627149ull},
};

// a^-1 mod q when gcd(a, q) = 1 (extended Euclid: q need not be prime)
static bool invert(uint64_t a, uint64_t q, uint64_t& out) {
    __int128 t = 0, nt = 1, r = q, nr = a % q;
    while (nr != 0) {
        const __int128 k = r / nr;
        __int128 x = t - k * nt; t = nt; nt = x;
        x = r - k * nr; r = nr; nr = x;
    }
    if (r != 1) return false;
    if (t < 0) t += q;
    out = (uint64_t)t;
    return true;
}

static int blocks(size_t work, unsigned cap = 256 * 32) {
    return (int)std::max<size_t>(1, std::min<size_t>((work + kLagBlock - 1) / kLagBlock, cap));
}

}  // namespace lsr

namespace lsr {

struct LagrangeProver {
    uint32_t m = 0, n_vars = 0;
    uint64_t q = 0;
    int device = 0;
    bool omega = false;                    // the quirk's domain {omega^j}
    MontQ M{};
    DeviceBuffer<uint32_t> row_ptr[3], col[3];
    DeviceBuffer<uint64_t> val[3];         // Montgomery form
    DeviceBuffer<uint64_t> lt;             // [m][m]: lt[i m + k] = L[k][i] 2^128
    DeviceBuffer<uint64_t> tser;           // [max(1, m - 1)]: T 2^128
    DeviceBuffer<uint64_t> zh_s, zh_m;     // [m + 1]: Z_H 2^128, Z_H 2^64
    std::mutex mutex;                      // guards the workspace and `stream`
    Stream stream;
    Event ev_last;                         // end of the last asynchronous call: the next call (any stream) starts behind it
    int chunk_log2 = 26;                   // LAMBDA_SNARK_QUOTIENT_CHUNK_LOG2, read once at creation
    // workspace for ws.chunk instances
    R1csScratch ws;                        // per-instance scratch and host staging
    DeviceBuffer<uint64_t> witness;        // [chunk][n_vars]
    DeviceBuffer<uint64_t> evals, coef;    // [3][chunk][m]
    DeviceBuffer<uint64_t> top;            // [chunk][max(1, m - 1)]
    DeviceBuffer<uint64_t> quot;           // [chunk][m]
    DeviceBuffer<uint64_t> qp, msg;        // [chunk][m + 1]
    DeviceBuffer<uint32_t> flags;          // bad[chunk] len[chunk]
};

// ---- plan tables, O(m^2) on the host ----------------------------------------------------------------------------------------
// Z = prod_j (X - x_j) over the domain; P_i = Z / (X - x_i) by synthetic division; P_i(x_i) = prod_{j != i} (x_i - x_j) = 1 / w_i;
// L[k][i] = w_i coef_k(P_i) (unique: any exact construction gives the reference's words).  Z_H = prod_{i<m} (X - i) always.
static std::vector<uint64_t> vanishing(const std::vector<uint64_t>& x, const MontQ& M) {
    std::vector<uint64_t> z(1, 1);
    for (uint64_t xj : x) {
        const uint64_t xm = mq_to(xj, M);
        z.push_back(0);
        for (size_t k = z.size() - 1; k > 0; --k) z[k] = mq_sub(z[k - 1], mq_mul(z[k], xm, M), M);
        z[0] = mq_sub(0, mq_mul(z[0], xm, M), M);
    }
    return z;
}

static bool build_tables(LagrangeProver& p, std::string& why) {
    const uint32_t m = p.m;
    const MontQ& M = p.M;
    const uint64_t q = p.q;
    std::vector<uint64_t> x(m);
    uint64_t omega = 0;
    if (q == kQuirkModulus)
        for (const auto& r : kQuirkRoots)
            if (r.m == m) omega = r.omega;
    p.omega = omega != 0;
    for (uint32_t j = 0; j < m; ++j) x[j] = omega ? (j ? mulmod(x[j - 1], omega, q) : 1) : (uint64_t)j % q;
    const std::vector<uint64_t> z = vanishing(x, M);
    std::vector<uint64_t> zh = p.omega ? vanishing([&] { std::vector<uint64_t> s(m); for (uint32_t j = 0; j < m; ++j) s[j] = j % q; return s; }(), M) : z;
    std::vector<uint64_t> lt((size_t)m * m), P(m);
    for (uint32_t i = 0; i < m; ++i) {
        const uint64_t xm = mq_to(x[i], M);
        P[m - 1] = z[m];                                                     // = 1
        for (uint32_t k = m - 1; k > 0; --k) P[k - 1] = mq_add(z[k], mq_mul(P[k], xm, M), M);
        uint64_t d = 0;                                                      // P_i(x_i) by Horner
        for (uint32_t k = m; k-- > 0;) d = mq_add(mq_mul(d, xm, M), P[k], M);
        uint64_t w;
        if (!invert(d, q, w)) {                                              // mod_inverse panics (arith.rs:66-85)
            why = "the interpolation denominator prod_{j != " + std::to_string(i) + "} (x_i - x_j) is not a unit mod q (the reference panics in mod_inverse)";
            return false;
        }
        const uint64_t ws = mulmod(w, M.r3, q);                              // w 2^192: mq_mul(P, ws) = w P 2^128
        for (uint32_t k = 0; k < m; ++k) lt[(size_t)i * m + k] = mq_mul(P[k], ws, M);
    }
    // T = 1 / rev(Z_H) mod X^(m-1): T_0 = 1, T_l = -sum_{j=1}^{l} zh[m-j] T_{l-j}
    const uint32_t w = std::max<uint32_t>(1, m - 1);
    std::vector<uint64_t> T(w, 0), ts(w, 0);
    T[0] = 1 % q;
    for (uint32_t l = 1; l + 1 < m; ++l) {
        Acc192 acc;
        acc_zero(acc);
        for (uint32_t j = 1; j <= l; ++j) acc_mac(acc, zh[m - j], T[l - j]);
        T[l] = mq_sub(0, mq_mul(acc_reduce(acc, M), M.r3, M), M);
    }
    for (uint32_t l = 0; l < w; ++l) ts[l] = mulmod(T[l], M.r2, q);
    std::vector<uint64_t> zs(m + 1), zm(m + 1);
    for (uint32_t k = 0; k <= m; ++k) {
        zs[k] = mulmod(zh[k], M.r2, q);
        zm[k] = mulmod(zh[k], M.r1, q);
    }
    p.lt.upload(lt);
    p.tser.upload(ts);
    p.zh_s.upload(zs);
    p.zh_m.upload(zm);
    return true;
}

void lagrange_destroy(LagrangeProver* p) {
    if (!p) return;
    try {
        DeviceGuard guard(p->device);
        p->ev_last.sync();
        delete p;
    } catch (...) {
        delete p;
    }
}

int lagrange_device(const LagrangeProver* p) { return p ? p->device : -1; }
bool lagrange_omega_domain(const LagrangeProver* p) { return p && p->omega; }

LagrangeProver* lagrange_create(const SparseMatrix* const mats[3], uint64_t q, int device) {
    const char* where = "lsr_r1cs_prover_create_mod";
    const uint32_t m = mats[0]->n_rows, n_vars = mats[0]->n_cols;
    if (q < 3 || (q & 1) == 0) {
        set_last_error(std::string(where) + ": the Lagrange path needs an odd modulus q >= 3 (for even q the reference succeeds only for m <= 2)");
        return nullptr;
    }
    if (m == 0 || m > kLagrangeMaxM) {
        set_last_error(std::string(where) + ": the Lagrange path takes 1 <= m <= 8192 constraints");
        return nullptr;
    }
    if (!r1cs_shape_ok(where, mats)) return nullptr;
    device = resolve_device(where, device, false);
    if (device < 0) return nullptr;
    LagrangeProverPtr p(new LagrangeProver);
    p->m = m;
    p->n_vars = n_vars;
    p->q = q;
    p->device = device;
    p->M = make_mont(q);
    if (const char* e = std::getenv("LAMBDA_SNARK_QUOTIENT_CHUNK_LOG2")) {
        const int v = std::atoi(e);
        if (v >= 1 && v <= 30) p->chunk_log2 = v;
    }
    try {
        DeviceGuard guard(device);
        std::string why;
        if (!build_tables(*p, why)) {
            set_last_error(std::string(where) + ": " + why);
            return nullptr;
        }
        const MontQ& M = p->M;
        upload_csr(mats, p->row_ptr, p->col, p->val, [&](uint64_t v) { return mq_to(v, M); });   // (val mod q) 2^64
        LSR_HIP(hipStreamCreateWithFlags(&p->stream.handle, hipStreamNonBlocking));
    } catch (const std::exception& e) {
        set_last_error(std::string(where) + ": " + e.what());
        return nullptr;
    }
    return p.release();
}

// ---- the pipeline ------------------------------------------------------------------------------------------------------------
static size_t chunk_for(const LagrangeProver& p, size_t batch) {
    return std::min(batch, std::max<size_t>(1, (size_t(1) << p.chunk_log2) / p.m));
}

static void ensure_workspace(LagrangeProver& p, size_t chunk, size_t n_public) {
    const size_t m = p.m, c = std::max(p.ws.chunk, chunk);
    p.witness.reserve(c * p.n_vars);
    p.evals.reserve(3 * c * m);
    p.coef.reserve(3 * c * m);
    p.top.reserve(c * std::max<size_t>(1, m - 1));
    p.quot.reserve(c * m);
    p.qp.reserve(c * (m + 1));
    p.msg.reserve(c * (m + 1));
    p.flags.reserve(2 * c);
    p.ws.grow(c, n_public);
}

// constraint evaluations of `count` witnesses (device, [count][n_vars]) into p.evals; interpolation into p.coef (interp); the
// quotient into p.quot with len [count] (quotient).  All on `s`.
static void run_chunk(LagrangeProver& p, const uint64_t* d_z, size_t count, bool interp, bool quotient, uint32_t* d_len, hipStream_t s) {
    const uint32_t m = p.m;
    const size_t per_vector = count * m;
    uint64_t* E = p.evals.ptr;
    uint64_t* Cf = p.coef.ptr;
    const LagCsr a{p.row_ptr[0].ptr, p.col[0].ptr, p.val[0].ptr}, b{p.row_ptr[1].ptr, p.col[1].ptr, p.val[1].ptr},
        c{p.row_ptr[2].ptr, p.col[2].ptr, p.val[2].ptr};
    hipLaunchKernelGGL(lag_constraint_evals_kernel, dim3(blocks(per_vector), 3), dim3(kLagBlock), 0, s, E, a, b, c, d_z, p.n_vars, m, per_vector, p.M);
    if (interp) {
        const size_t rows = 3 * count;
        const unsigned row_tiles = (unsigned)((rows + kGemmTile - 1) / kGemmTile);
        if (m <= (uint32_t)kSmallMaxM)
            hipLaunchKernelGGL(lag_interp_small_kernel, dim3(row_tiles), dim3(kLagBlock), 0, s, E, p.lt.ptr, Cf, rows, m, p.M);
        else
            hipLaunchKernelGGL(lag_interp_tiled_kernel, dim3(row_tiles, (m + kGemmTile - 1) / kGemmTile), dim3(kLagBlock), 0, s, E, p.lt.ptr, Cf, rows, m, p.M);
    }
    if (quotient) {
        uint32_t* bad = p.flags.ptr;
        LSR_HIP(hipMemsetAsync(bad, 0, count * sizeof(uint32_t), s));
        hipLaunchKernelGGL(lag_check_kernel, dim3(blocks(per_vector)), dim3(kLagBlock), 0, s, E, E + per_vector, E + 2 * per_vector, bad, m, per_vector, p.M);
        if (m >= 2)
            hipLaunchKernelGGL(lag_top_kernel, dim3(blocks(count * (m - 1))), dim3(kLagBlock), 0, s, Cf, Cf + per_vector, p.top.ptr, m,
                               count * (m - 1), p.M);
        hipLaunchKernelGGL(lag_toeplitz_kernel, dim3(blocks(per_vector)), dim3(kLagBlock), 0, s, p.top.ptr, p.tser.ptr, p.quot.ptr, m, per_vector, p.M);
        if (p.omega)   // on {0..m-1} is_satisfied already implies Z_H | N
            hipLaunchKernelGGL(lag_remainder_kernel, dim3(blocks(per_vector)), dim3(kLagBlock), 0, s, Cf, Cf + per_vector, Cf + 2 * per_vector, p.quot.ptr,
                               p.zh_s.ptr, bad, m, per_vector, p.M);
        hipLaunchKernelGGL(lag_len_kernel, dim3(blocks(count, ~0u)), dim3(kLagBlock), 0, s, p.quot.ptr, bad, d_len, m, count);
    }
    LSR_HIP(hipGetLastError());
}

void lagrange_host_run(LagrangeProver& p, const uint64_t* w, size_t batch, uint64_t* const evals[3], uint64_t* const coeffs[3], uint64_t* quotient,
                       uint32_t* len) {
    DeviceGuard guard(p.device);
    std::lock_guard<std::mutex> lock(p.mutex);
    p.ev_last.sync();
    const size_t chunk = chunk_for(p, batch);
    ensure_workspace(p, chunk, 0);
    hipStream_t s = p.stream;
    uint32_t* d_len = p.flags.ptr + p.ws.chunk;
    for (size_t done = 0; done < batch; done += chunk) {
        const size_t now = std::min(chunk, batch - done);
        const size_t per_vector = now * p.m, off = done * p.m;
        LSR_HIP(hipMemcpyAsync(p.witness.ptr, w + done * p.n_vars, now * p.n_vars * 8, hipMemcpyHostToDevice, s));
        run_chunk(p, p.witness.ptr, now, !evals, !evals && !coeffs, d_len, s);
        if (evals || coeffs) {
            const uint64_t* src = evals ? p.evals.ptr : p.coef.ptr;
            uint64_t* const* dst = evals ? evals : coeffs;
            for (int k = 0; k < 3; ++k) LSR_HIP(hipMemcpyAsync(dst[k] + off, src + k * per_vector, per_vector * 8, hipMemcpyDeviceToHost, s));
        } else {
            LSR_HIP(hipMemcpyAsync(quotient + off, p.quot.ptr, per_vector * 8, hipMemcpyDeviceToHost, s));
            LSR_HIP(hipMemcpyAsync(len + done, d_len, now * 4, hipMemcpyDeviceToHost, s));
        }
        LSR_HIP(hipStreamSynchronize(s));
    }
}

// one chunk of prove_r1cs / prove_r1cs_zk: evaluations -> interpolation -> quotient -> message -> keys -> rows -> alpha -> beta ->
// evaluations at alpha and beta -> proof records
static void prove_chunk(LagrangeProver& p, const R1csProveCall& a, const uint64_t* d_z, const uint64_t* d_blind, const uint64_t* seeds, size_t count,
                        uint64_t* d_rows, uint64_t* d_proofs, uint8_t* d_hashes, uint32_t* d_status, bool host_keys, hipStream_t s) {
    const uint32_t m = p.m;
    const size_t per_vector = count * m;
    const size_t words = lsr_lwe_commitment_words(a.lwe);
    const R1csSlots v = p.ws.slots();
    uint32_t* d_len = p.flags.ptr + p.ws.chunk;
    run_chunk(p, d_z, count, true, true, d_len, s);
    const uint32_t msg_len = m + (d_blind ? 1u : 0u);
    hipLaunchKernelGGL(lag_message_kernel, dim3(blocks(count * (m + 1))), dim3(kLagBlock), 0, s, p.quot.ptr, d_blind, p.zh_m.ptr, p.qp.ptr, p.msg.ptr,
                       msg_len, a.commit_modulus, m, count * (size_t)(m + 1), p.M);
    LSR_HIP(hipGetLastError());
    commit_messages(a.lwe, p.msg.ptr, msg_len, count, seeds, v.keys, d_rows, host_keys, s);
    r1cs_transcript(lag_gather_publics_kernel, v, d_z, p.n_vars, a.n_public, d_rows, words, count, p.q, s);
    LagEvalPolys polys;
    for (int k = 0; k < 3; ++k) {
        polys.poly[k] = p.coef.ptr + k * per_vector;
        polys.stride[k] = m;
        polys.len[k] = m;
    }
    polys.poly[3] = p.qp.ptr;
    polys.stride[3] = m + 1;
    polys.len[3] = m + 1;
    hipLaunchKernelGGL(lag_eval_kernel, dim3((unsigned)count, 4), dim3(64), 0, s, polys, v.alphas, v.betas, v.ev, p.M);
    hipLaunchKernelGGL(lag_assemble_kernel, dim3(blocks(count, ~0u)), dim3(kLagBlock), 0, s, v.ev, v.alphas, v.betas, d_blind, d_len, v.hash_a, v.hash_b,
                       d_proofs, reinterpret_cast<uint64_t*>(d_hashes), d_status, count, p.q);
    LSR_HIP(hipGetLastError());
}

void lagrange_prove(LagrangeProver& p, const R1csProveCall& c, bool on_device, hipStream_t s) {
    const R1csProverRef ref{p.device, p.mutex, p.ev_last, p.stream, p.witness, p.n_vars, p.ws};
    const auto grow = [&](size_t chunk) { ensure_workspace(p, chunk, c.n_public); };
    const auto chunk = [&](auto... args) { prove_chunk(p, c, args...); };
    if (on_device) r1cs_prove_device(ref, c, chunk_for(p, c.batch), grow, chunk, s);
    else r1cs_prove_host(ref, c, chunk_for(p, c.batch), grow, chunk);
}

// ---- verify on the baseline path ---------------------------------------------------------------------------------------------
void verify_mod_host(uint32_t m, uint64_t q, const uint64_t* pub, size_t n_public, const uint64_t* rows, size_t words, const uint64_t* proofs,
                     size_t batch, bool zk, int* results) {
    const MontQ M = make_mont(q);
    r1cs_verify_host(q, pub, n_public, rows, words, proofs, batch, results,
                     [&](const uint64_t* proof, uint64_t alpha, uint64_t beta) { return verify_one_generic(proof, alpha, beta, m, zk, M); });
}

void verify_mod_device(uint32_t m, uint64_t q, const uint64_t* d_pub, size_t n_public, const uint64_t* d_rows, size_t words, const uint64_t* d_proofs,
                       size_t batch, bool zk, int* d_results, hipStream_t s) {
    r1cs_verify_device(q, d_pub, n_public, d_rows, words, batch, s, [&](const uint64_t* d_alphas, const uint64_t* d_betas) {
        hipLaunchKernelGGL(lag_verify_kernel, dim3(blocks(batch, ~0u)), dim3(kLagBlock), 0, s, d_proofs, d_alphas, d_betas, m, zk ? 1 : 0, d_results, batch,
                           make_mont(q));
    });
}

}  // namespace lsr
