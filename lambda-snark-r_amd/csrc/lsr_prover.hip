// Prover-side polynomial path on the NTT kernels: natural-order cyclic transforms (rust-api/lambda-snark/src/ntt.rs)
// and the NTT-path quotient polynomial (rust-api/lambda-snark/src/r1cs.rs:474-506).  C-ABI in lambda_snark/prover.h.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "lambda_snark/prover.h"
#include "lambda_snark/batch.h"
#include "lsr_lagrange.hpp"
#include "lsr_prove_common.hpp"
#include "lsr_prove_kernels.hpp"
#include "lsr_runtime.hpp"

namespace lsr {

constexpr int kBlock = 256;

static unsigned blocks_for(size_t work, unsigned cap = 256 * 32) {
    return static_cast<unsigned>(std::max<size_t>(1, std::min<size_t>((work + kBlock - 1) / kBlock, cap)));
}

__device__ __forceinline__ uint64_t gold_canon(uint64_t x) { return x >= kGoldilocks ? x - kGoldilocks : x; }

// ---- quotient pipeline -------------------------------------------------------------------------------------------
// r1cs.rs:489-503 computes N = A B - C from the interpolated polynomials and divides by Z_H = X^m - 1, failing when a
// remainder is left.  Equivalent, with transforms of size m only:
//   * the remainder vanishes iff N vanishes on H = {omega^k}, i.e. iff a_k b_k = c_k for every constraint k;
//   * then Q = N / Z_H has degree <= m - 2, so it is fixed by its values on the coset psi H (psi = omega_2m, psi^2 = omega),
//     where Z_H(psi omega^k) = psi^m - 1 = -2:   Q(psi omega^k) = (A B - C)(psi omega^k) / (-2).
// Radix-2 in-place networks permute by bit reversal (P).  With F_w the DFT matrix of root w and a context built on the
// CONJUGATE root omega^-1, the two launches are
//      forward = P F_{1/omega}           : natural-order values -> m x (inverse DFT), bit-reversed
//      inverse = (P F_{1/omega})^-1      = m^-1 F_omega P : bit-reversed coefficients -> natural-order evaluations
// so  e --forward--> m P coeffs --[x psi^bitrev(p) fused into the read-in]--inverse--> evaluations on psi H (natural order)
// needs no permutation and no scaling, and the way back is forward again.
// C enters linearly, so it never goes to the coset: modulo X^m + 1 (whose roots are psi H) Z_H = -2 and C is its own
// remainder, hence Q = (C - (A B mod X^m + 1)) / 2 coefficient by coefficient.  Six transforms in all: A, B, C interpolated
// (c^ = m P c stays where it is), A and B evaluated on the coset and multiplied, one transform back (z = m P (psi^j g_j)_j
// with g = A B mod X^m + 1), and the finish Q_j = (2m)^-1 (c^[p] - psi^-j z[p]), p = bitrev(j) — the only place where m
// words are put in natural order (through LDS).

// test a_k b_k = c_k (is_satisfied, r1cs.rs:148-172) — the first transform reads the evaluations where they lie
__global__ void __launch_bounds__(kBlock) check_kernel(const uint64_t* __restrict__ a, const uint64_t* __restrict__ b, const uint64_t* __restrict__ c,
                                                       uint32_t* __restrict__ bad, int logm, size_t per_vector) {
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t base = (size_t)blockIdx.x * kBlock; base < per_vector; base += stride) {   // wave-uniform trip count
        const size_t i = base + threadIdx.x;
        const bool live = i < per_vector;
        bool wrong = false;
        if (live) {
            wrong = gold_mul(gold_canon(a[i]), gold_canon(b[i])) != gold_canon(c[i]);
        }
        if (logm >= 6) {   // a wavefront's 64 consecutive constraints belong to one instance
            if (__ballot(wrong) && (threadIdx.x & 63) == 0) atomicOr(&bad[i >> logm], 1u);
        } else if (wrong) {
            atomicOr(&bad[i >> logm], 1u);
        }
    }
}

// the prove path's stash of A's and B's interpolated planes: 16-byte words, grid-stride (a device-to-device hipMemcpyAsync took
// 7x as long on the same planes)
__global__ void __launch_bounds__(kBlock) stash_kernel(const ulonglong2* __restrict__ src, ulonglong2* __restrict__ dst, size_t count) {
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += stride) dst[i] = src[i];
}

// evaluations of A B on the coset, written over A's
__global__ void __launch_bounds__(kBlock) product_kernel(uint64_t* __restrict__ a, const uint64_t* __restrict__ b, size_t count) {
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += stride) a[i] = gold_mul(a[i], b[i]);
}

// compute_constraint_evals (r1cs.rs:296-304): out[mat][inst][row] = sum_e val[e] * z[inst][col[e]] over the row's CSR run.
// One lane per (instance, row); blockIdx.y selects the matrix.  Witness words may be any 64-bit value (v[col] % modulus).
struct CsrView {
    const uint32_t* row_ptr;   // [m + 1]
    const uint32_t* col;
    const uint64_t* val;       // value mod q, in Montgomery form
};
__global__ void __launch_bounds__(kBlock) constraint_evals_kernel(uint64_t* __restrict__ out, CsrView a, CsrView b, CsrView c,
                                                                  const uint64_t* __restrict__ z, uint32_t n_vars, int logm, size_t per_vector) {
    const CsrView mat = blockIdx.y == 0 ? a : (blockIdx.y == 1 ? b : c);
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < per_vector; i += stride) {
        const uint32_t row = (uint32_t)i & ((1u << logm) - 1u);
        const uint64_t* zi = z + (i >> logm) * n_vars;
        uint64_t acc = 0;
        for (uint32_t e = mat.row_ptr[row]; e < mat.row_ptr[row + 1]; ++e) acc = gold_add(acc, gold_mul_mont(zi[mat.col[e]], mat.val[e]));
        out[blockIdx.y * per_vector + i] = acc;
    }
}

constexpr int kSplitTile = 4096;                 // quotient words per workgroup
constexpr int kSplitPerThread = kSplitTile / kBlock;
__device__ __forceinline__ int split_slot(int i) { return i + (i >> 6); }   // one pad word per 64

// z, chat = [instances][m] in bit-reversed order -> quotient[inst][j] = half_m_inv * chat[inst][p] - untwist[p] * z[inst][p],
// p = bitrev(j), untwist[p] = (2m)^-1 psi^-bitrev(p) (both multipliers in Montgomery form); and per instance `top` =
// 1 + highest non-zero index.
// LOGM_HIGH: m >= 4096, one workgroup moves the 4096 words whose index has a fixed middle field (bits 6..logm-7):
// 64-word runs on both the read and the write side.
template <bool LOGM_HIGH>
__global__ void __launch_bounds__(kBlock) finish_quotient_kernel(const uint64_t* __restrict__ z, const uint64_t* __restrict__ chat,
                                                                 const uint64_t* __restrict__ untwist, uint64_t half_m_inv,
                                                                 uint64_t* __restrict__ quotient, uint32_t* __restrict__ top, int logm, size_t total) {
    __shared__ uint64_t tile[kSplitTile + kSplitTile / 64];
    const int t = threadIdx.x;
    const uint32_t mmask = (1u << logm) - 1u;
    if constexpr (LOGM_HIGH) {
        // bit-reversed-order index (A:6 | B | C:6)  ->  natural index (rev C | rev B | rev A)
        const int mid_bits = logm - 12;
        const size_t inst = blockIdx.x >> mid_bits;
        const uint32_t B = blockIdx.x & ((1u << mid_bits) - 1u);
        const uint32_t Brev = mid_bits ? (__brev(B) >> (32 - mid_bits)) : 0u;
        const int lane = t & 63, wave = t >> 6;
#pragma unroll
        for (int r = 0; r < kSplitPerThread; ++r) {
            const int A = wave * kSplitPerThread + r;
            const uint32_t pidx = ((uint32_t)A << (logm - 6)) | (B << 6) | (uint32_t)lane;
            const size_t g = (inst << logm) + pidx;
            tile[A * 65 + lane] = gold_sub(gold_mul_mont(chat[g], half_m_inv), gold_mul_mont(z[g], untwist[pidx]));
        }
        __syncthreads();
        uint32_t best = 0;
#pragma unroll
        for (int r = 0; r < kSplitPerThread; ++r) {
            const int Cout = wave * kSplitPerThread + r;              // top field of the natural index
            const uint32_t nat = ((uint32_t)Cout << (logm - 6)) | (Brev << 6) | (uint32_t)lane;
            const uint64_t h = tile[(__brev((uint32_t)lane) >> 26) * 65 + (__brev((uint32_t)Cout) >> 26)];
            quotient[(inst << logm) + nat] = h;
            if (h != 0) best = nat + 1;                                // nat grows with r within a thread
        }
        for (int off = 32; off; off >>= 1) best = max(best, (uint32_t)__shfl_xor((int)best, off));
        if (best && lane == 0) atomicMax(&top[inst], best);
    } else {
        // m < 4096: the tile holds 2^(12-logm) whole instances; scatter into LDS, stream out in natural order
        const size_t tile_base = (size_t)blockIdx.x * kSplitTile;
#pragma unroll
        for (int r = 0; r < kSplitPerThread; ++r) {
            const int p = r * kBlock + t;
            const size_t g = tile_base + p;
            if (g < total) {
                const uint32_t j = (uint32_t)p & mmask;
                const uint32_t nat = logm ? (__brev(j) >> (32 - logm)) : 0u;
                tile[split_slot((p & ~(int)mmask) | (int)nat)] = gold_sub(gold_mul_mont(chat[g], half_m_inv), gold_mul_mont(z[g], untwist[j]));
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < kSplitPerThread; ++r) {
            const int p = r * kBlock + t;
            const size_t g = tile_base + p;
            const bool live = g < total;
            const uint32_t nat = (uint32_t)p & mmask;
            uint64_t h = 0;
            if (live) {
                h = tile[split_slot(p)];
                quotient[g] = h;
            }
            if (logm >= 6) {   // a wavefront's 64 consecutive words belong to one instance: one atomic per wave
                const uint64_t nz = __ballot(live && h != 0);
                if (nz && (t & 63) == 63 - __clzll(nz)) atomicMax(&top[g >> logm], nat + 1);
            } else if (live && h != 0) {
                atomicMax(&top[g >> logm], nat + 1);
            }
        }
    }
}

__global__ void __launch_bounds__(kBlock) quotient_len_kernel(uint32_t* __restrict__ len, const uint32_t* __restrict__ top,
                                                              const uint32_t* __restrict__ bad, size_t batch) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < batch) len[i] = bad[i] ? 0u : (top[i] ? top[i] : 1u);
}

}  // namespace lsr

struct LsrQuotientPlan {
    uint32_t m = 0;
    int logm = 0;
    int device = 0;
    lsr::NttContextPtr ntt;                   // size m, on the conjugate root omega_m^-1 (absent for m = 1); released after the buffers
    lsr::DeviceBuffer<uint64_t> twist;        // psi^bitrev(p), p < m                  } all three in Montgomery form
    lsr::DeviceBuffer<uint64_t> untwist;      // (2m)^-1 psi^-bitrev(p), p < m         } (gold_mul_mont)
    uint64_t half_m_inv = 0;                  // (2m)^-1                               }
    std::mutex mutex;                         // guards the workspace and `stream`
    lsr::DeviceBuffer<uint64_t> work;         // [3][chunk][m]
    lsr::DeviceBuffer<uint32_t> flags;        // top[chunk], bad[chunk]
    lsr::DeviceBuffer<uint64_t> io;           // host-API staging of the quotient: [chunk][m]
    lsr::DeviceBuffer<uint32_t> io_len;
    size_t chunk = 0;                         // instances the planes are laid out for (committed once they are allocated)
    lsr::Stream stream;
    lsr::Event ev_last;                       // end of the last asynchronous call: the next call on this plan (any stream) starts behind it
    // read from the environment ONCE, when the plan is created
    int chunk_log2 = 26;                      // LAMBDA_SNARK_QUOTIENT_CHUNK_LOG2: evaluations per pass and plane
    bool fuse = true;                         // LAMBDA_SNARK_QUOTIENT_FUSE=0: the a b = c test and the coset product as kernels of their own
};

namespace lsr {

// instances per pass: bound the workspace (3 m words per instance; 2^26 evaluations per vector ~ 1.5 GiB; p.chunk_log2: tests force
// several passes with LAMBDA_SNARK_QUOTIENT_CHUNK_LOG2 at plan creation)
static size_t quotient_chunk(const LsrQuotientPlan& p, size_t batch) {
    const size_t cap = std::max<size_t>(1, (size_t(1) << p.chunk_log2) >> p.logm);
    return std::min(batch, cap);
}

static void ensure_workspace(LsrQuotientPlan& p, size_t chunk, bool host_io) {
    const size_t c = std::max(p.chunk, chunk);
    if (c > p.chunk) {          // the host staging follows the planes' layout: dropped, re-made by the next host call
        p.io.release();
        p.io_len.release();
    }
    p.work.reserve(3 * c * p.m);
    p.flags.reserve(2 * c);
    if (host_io) {
        p.io.reserve(c * p.m);
        p.io_len.reserve(c);
    }
    p.chunk = c;
}

// one pass over `count` <= plan.chunk instances, everything on `s`
// stash (prove path, in-place calls only): receives [2][count][m] — A's and B's interpolated planes (m P coeffs) before the coset
// transform overwrites them; C's stays in the third plane
static void quotient_pass(LsrQuotientPlan& p, const uint64_t* d_a, const uint64_t* d_b, const uint64_t* d_c, size_t count, uint64_t* d_q,
                          uint32_t* d_len, hipStream_t s, uint64_t* stash = nullptr) {
    const size_t per_vector = count << p.logm;
    uint64_t* work = p.work.ptr;
    uint32_t* top = p.flags.ptr;
    uint32_t* bad = p.flags.ptr + count;
    zero_words_async(reinterpret_cast<uint64_t*>(p.flags.ptr), count, s);                 // top[count], bad[count]: 2 count u32 = count words
    // m <= 4096 (one tile launch per transform): the two elementwise kernels ride in the read-in of a transform — the a b = c test in
    // C's interpolation, the coset product in the last transform (the transforms are integer-VALU-bound, the extra loads cost nothing
    // and two passes over the planes disappear: profiles/r02b_quotient_fusion.txt).  A plan created under LAMBDA_SNARK_QUOTIENT_FUSE=0 keeps them apart.
    const bool fuse = p.fuse && p.ntt && ntt_forward_can_fuse(*p.ntt);
    const bool fuse_check = fuse && d_a != work;
    if (!fuse_check) hipLaunchKernelGGL(check_kernel, dim3(blocks_for(per_vector)), dim3(kBlock), 0, s, d_a, d_b, d_c, bad, p.logm, per_vector);
    if (p.ntt) {
        if (d_a == work) {                                                               // interpolation: r1cs.rs:489-491
            launch_ntt(*p.ntt, work, 3 * count, false, s);
            if (stash) hipLaunchKernelGGL(stash_kernel, dim3(blocks_for(per_vector)), dim3(kBlock), 0, s, reinterpret_cast<const ulonglong2*>(work),
                                          reinterpret_cast<ulonglong2*>(stash), per_vector);   // 2 per_vector words
        } else {   // out of place: the caller's arrays are read, the workspace planes written
            launch_ntt(*p.ntt, work, count, false, s, nullptr, nullptr, d_a);
            launch_ntt(*p.ntt, work + per_vector, count, false, s, nullptr, nullptr, d_b);
            if (fuse_check) launch_ntt_forward_fused(*p.ntt, work + 2 * per_vector, count, s, d_c, 2, d_a, d_b, bad);
            else launch_ntt(*p.ntt, work + 2 * per_vector, count, false, s, nullptr, nullptr, d_c);
        }
        launch_ntt(*p.ntt, work, 2 * count, true, s, nullptr, p.twist.ptr);              // A, B on the coset psi H
        if (fuse) {
            // (a b) -> coefficients (r1cs.rs:495) and the finish below in one launch: the product rides in the transform's read-in, the
            // subtraction of c, the untwist, the bit reversal and the degree bound in its write-out (lsr_ntt_kernels.hpp, MODE 3)
            launch_ntt_forward_finish(*p.ntt, work, count, s, work + per_vector, work + 2 * per_vector, p.untwist.ptr, p.half_m_inv, d_q, top);
        } else {
            hipLaunchKernelGGL(product_kernel, dim3(blocks_for(per_vector)), dim3(kBlock), 0, s, work, work + per_vector, per_vector);   // r1cs.rs:495
            launch_ntt(*p.ntt, work, count, false, s);                                   // back to (twisted, bit-reversed) coefficients
        }
        if (fuse) {
        } else if (p.logm >= 12) {
            hipLaunchKernelGGL(finish_quotient_kernel<true>, dim3(static_cast<unsigned>(per_vector / kSplitTile)), dim3(kBlock), 0, s, work,
                               work + 2 * per_vector, p.untwist.ptr, p.half_m_inv, d_q, top, p.logm, per_vector);
        } else {
            hipLaunchKernelGGL(finish_quotient_kernel<false>, dim3(static_cast<unsigned>((per_vector + kSplitTile - 1) / kSplitTile)), dim3(kBlock), 0, s,
                               work, work + 2 * per_vector, p.untwist.ptr, p.half_m_inv, d_q, top, p.logm, per_vector);
        }
    } else {
        zero_words_async(d_q, per_vector, s);                                            // m = 1: constants, Q = 0 when a b = c
        if (stash) hipLaunchKernelGGL(stash_kernel, dim3(blocks_for(per_vector)), dim3(kBlock), 0, s, reinterpret_cast<const ulonglong2*>(work),
                                          reinterpret_cast<ulonglong2*>(stash), per_vector);   // 2 per_vector words
    }
    hipLaunchKernelGGL(quotient_len_kernel, dim3(blocks_for(count, ~0u)), dim3(kBlock), 0, s, d_len, top, bad, count);
    LSR_HIP(hipGetLastError());
}

static void quotient_device(LsrQuotientPlan& p, const uint64_t* d_a, const uint64_t* d_b, const uint64_t* d_c, size_t batch, uint64_t* d_q,
                            uint32_t* d_len, hipStream_t s) {
    DeviceGuard guard(p.device);
    std::lock_guard<std::mutex> lock(p.mutex);
    // the workspace planes are the plan's: calls on one plan run one behind the other whatever streams the caller passes (and a
    // workspace about to grow is not freed under a call that still uses it)
    // (not while `s` records into a HIP graph: a captured sequence is ordered by the capture, lsr_runtime.hpp stream_is_capturing)
    const bool capturing = stream_is_capturing(s);
    if (!capturing) p.ev_last.sync();
    const size_t chunk = quotient_chunk(p, batch);
    ensure_workspace(p, chunk, false);
    for (size_t done = 0; done < batch; done += chunk) {
        const size_t now = std::min(chunk, batch - done);
        const size_t off = done << p.logm;
        quotient_pass(p, d_a + off, d_b + off, d_c + off, now, d_q + off, d_len + done, s);
    }
    if (!capturing) p.ev_last.record(s);
}

static void quotient_host(LsrQuotientPlan& p, const uint64_t* a, const uint64_t* b, const uint64_t* c, size_t batch, uint64_t* q, uint32_t* len) {
    DeviceGuard guard(p.device);
    std::lock_guard<std::mutex> lock(p.mutex);
    p.ev_last.sync();      // an asynchronous call still using the planes
    const size_t chunk = quotient_chunk(p, batch);
    ensure_workspace(p, chunk, true);
    for (size_t done = 0; done < batch; done += chunk) {
        const size_t now = std::min(chunk, batch - done);
        const size_t off = done << p.logm, words = now << p.logm, bytes = words * 8;
        // straight into the workspace planes: the check then runs in place, without the device-side copy
        LSR_HIP(hipMemcpyAsync(p.work.ptr, a + off, bytes, hipMemcpyHostToDevice, p.stream));
        LSR_HIP(hipMemcpyAsync(p.work.ptr + words, b + off, bytes, hipMemcpyHostToDevice, p.stream));
        LSR_HIP(hipMemcpyAsync(p.work.ptr + 2 * words, c + off, bytes, hipMemcpyHostToDevice, p.stream));
        quotient_pass(p, p.work.ptr, p.work.ptr + words, p.work.ptr + 2 * words, now, p.io.ptr, p.io_len.ptr, p.stream);
        LSR_HIP(hipMemcpyAsync(q + off, p.io.ptr, bytes, hipMemcpyDeviceToHost, p.stream));
        LSR_HIP(hipMemcpyAsync(len + done, p.io_len.ptr, now * sizeof(uint32_t), hipMemcpyDeviceToHost, p.stream));
        LSR_HIP(hipStreamSynchronize(p.stream));
    }
}

static void destroy_plan(LsrQuotientPlan* p) {
    if (!p) return;
    try {
        DeviceGuard guard(p->device);
        p->ev_last.sync();
        delete p;
    } catch (...) {
        delete p;
    }
}
using QuotientPlanPtr = std::unique_ptr<LsrQuotientPlan, HandleDeleter<LsrQuotientPlan, destroy_plan>>;

// large: the ceiling is 2^22 (lsr_quotient_plan_create_large, the R1CS prover) instead of 2^17; `where` names the entry point
static LsrQuotientPlan* create_plan(uint32_t m, int device, bool large, const char* where) {
    const uint32_t max_m = 1u << (large ? kProverMaxLog2 : kTwoPassMaxLog2);
    if (m == 0 || m > max_m || (m & (m - 1))) {
        set_last_error(std::string(where) + ": m must be a power of two in [1, " + std::to_string(max_m) + "] (r1cs.rs:386-389)");
        return nullptr;
    }
    device = resolve_device(where, device, true);
    if (device < 0) return nullptr;
    QuotientPlanPtr p(new LsrQuotientPlan);
    p->m = m;
    p->device = device;
    if (const char* e = std::getenv("LAMBDA_SNARK_QUOTIENT_CHUNK_LOG2")) {
        const int v = std::atoi(e);
        if (v >= 1 && v <= 30) p->chunk_log2 = v;
    }
    if (const char* e = std::getenv("LAMBDA_SNARK_QUOTIENT_FUSE")) p->fuse = !(e[0] == '0');
    while ((1u << p->logm) < m) ++p->logm;
    const uint64_t q = kProverModulus;
    if (m >= 2) {
        p->ntt.reset(create_cyclic_ntt_context(q, m, invmod_prime(prover_root_of_unity(q, m), q), device, large, where));
        if (!p->ntt) return nullptr;
    }
    try {
        DeviceGuard guard(device);
        if (m >= 2) {
            const uint64_t psi = prover_root_of_unity(q, 2ull * m), psi_inv = invmod_prime(psi, q);
            std::vector<uint64_t> twist(m), untwist(m);
            const uint64_t half_m_inv = invmod_prime((2ull * m) % q, q);
            p->half_m_inv = prover_montgomery(half_m_inv);
            // The plan's own context transforms WITHOUT the m^-1 of its inverse direction (both scaling constants 1: the last stage then
            // costs no product, ArithGold::gs_scaled).  A and B reach the coset m times too large, their product and z carry m^2, and the
            // untwist table takes it back: untwist[p] = (2m)^-1 m^-2 psi^-bitrev(p).  (The context is private to the plan; the cyclic
            // transforms of lsr_cyclic_ntt_* use contexts of their own.)
            p->ntt->n_inv_gold = prover_montgomery(1);
            p->ntt->w_last_scaled_gold = prover_montgomery(1);       // the last stage's twiddle is omega^0
            const uint64_t m_inv = invmod_prime(m % q, q);
            uint64_t up = 1, down = mulmod(half_m_inv, mulmod(m_inv, m_inv, q), q);
            for (uint32_t j = 0; j < m; ++j) {
                twist[bit_reverse(j, p->logm)] = prover_montgomery(up);
                untwist[bit_reverse(j, p->logm)] = prover_montgomery(down);
                up = mulmod(up, psi, q);
                down = mulmod(down, psi_inv, q);
            }
            p->twist.upload(twist);
            p->untwist.upload(untwist);
        }
        LSR_HIP(hipStreamCreateWithFlags(&p->stream.handle, hipStreamNonBlocking));
    } catch (const std::exception& e) {
        set_last_error(std::string(where) + ": " + e.what());
        return nullptr;
    }
    return p.release();
}

}  // namespace lsr

struct LsrR1csProver {
    uint32_t m = 0, n_vars = 0;
    // (declared before the buffers: released after them)
    lsr::QuotientPlanPtr plan;              // NTT path
    lsr::LagrangeProverPtr lag;             // Lagrange path (lsr_r1cs_prover_create_mod, lsr_lagrange.hip): then plan == nullptr
    uint64_t modulus = lsr::kProverModulus;
    lsr::DeviceBuffer<uint32_t> row_ptr[3], col[3];
    lsr::DeviceBuffer<uint64_t> val[3];
    lsr::DeviceBuffer<uint64_t> witness;    // [chunk][n_vars]
    // prove path (lsr_r1cs_prove_batch*), sized for prove_chunk instances:
    lsr::DeviceBuffer<uint64_t> stash;      // A's and B's interpolated planes [2][chunk][m]
    lsr::DeviceBuffer<uint64_t> quot;       // quotient [chunk][m]
    lsr::DeviceBuffer<uint64_t> msg;        // commitment messages [chunk][m + 1]
    lsr::DeviceBuffer<uint32_t> len;        // [chunk]
    lsr::DeviceBuffer<uint64_t> eval_part;  // m > 2^17: per-slice sums of the evaluation stage [chunk][slices <= 1024][3][2]
    lsr::R1csScratch ws;                    // per-instance scratch and host staging; its chunk sizes the buffers above
    int device() const { return plan ? plan->device : lsr::lagrange_device(lag.get()); }
};

namespace lsr {

static void destroy_prover(LsrR1csProver* r) {
    if (!r) return;
    try {
        DeviceGuard guard(r->device());
        if (r->plan) r->plan->ev_last.sync();   // an asynchronous prove call still using the buffers below
        delete r;
    } catch (...) {
        delete r;
    }
}
using R1csProverPtr = std::unique_ptr<LsrR1csProver, HandleDeleter<LsrR1csProver, destroy_prover>>;

static LsrR1csProver* create_prover(const SparseMatrix* const mats[3], int device) {
    if (!r1cs_shape_ok("lsr_r1cs_prover_create", mats)) return nullptr;
    QuotientPlanPtr plan(create_plan(mats[0]->n_rows, device, true, "lsr_r1cs_prover_create"));
    if (!plan) return nullptr;
    R1csProverPtr r(new LsrR1csProver);
    r->m = mats[0]->n_rows;
    r->n_vars = mats[0]->n_cols;
    r->plan = std::move(plan);
    try {
        DeviceGuard guard(r->plan->device);
        upload_csr(mats, r->row_ptr, r->col, r->val, [](uint64_t v) { return prover_montgomery(v); });   // mul_vec: val % modulus (held in Montgomery form)
    } catch (const std::exception& e) {
        set_last_error(std::string("lsr_r1cs_prover_create: ") + e.what());
        return nullptr;
    }
    return r.release();
}

// witnesses (host) -> constraint evaluations in the plan's workspace planes, chunk by chunk; then either copy them out
// (evals != nullptr) or run the quotient pipeline on them in place
static void prover_run(LsrR1csProver& r, const uint64_t* witnesses, size_t batch, uint64_t* const evals[3], uint64_t* q, uint32_t* len) {
    LsrQuotientPlan& p = *r.plan;
    DeviceGuard guard(p.device);
    std::lock_guard<std::mutex> lock(p.mutex);
    p.ev_last.sync();      // an asynchronous lsr_quotient_batch_device call still using the planes
    const size_t chunk = quotient_chunk(p, batch);
    ensure_workspace(p, chunk, true);
    r.witness.reserve(p.chunk * r.n_vars);
    const CsrView a{r.row_ptr[0].ptr, r.col[0].ptr, r.val[0].ptr}, b{r.row_ptr[1].ptr, r.col[1].ptr, r.val[1].ptr},
        c{r.row_ptr[2].ptr, r.col[2].ptr, r.val[2].ptr};
    for (size_t done = 0; done < batch; done += chunk) {
        const size_t now = std::min(chunk, batch - done);
        const size_t per_vector = now << p.logm, off = done << p.logm;
        LSR_HIP(hipMemcpyAsync(r.witness.ptr, witnesses + done * r.n_vars, now * r.n_vars * 8, hipMemcpyHostToDevice, p.stream));
        hipLaunchKernelGGL(constraint_evals_kernel, dim3(blocks_for(per_vector), 3), dim3(kBlock), 0, p.stream, p.work.ptr, a, b, c, r.witness.ptr,
                           r.n_vars, p.logm, per_vector);
        LSR_HIP(hipGetLastError());
        if (evals) {
            for (int k = 0; k < 3; ++k)
                LSR_HIP(hipMemcpyAsync(evals[k] + off, p.work.ptr + k * per_vector, per_vector * 8, hipMemcpyDeviceToHost, p.stream));
        } else {
            quotient_pass(p, p.work.ptr, p.work.ptr + per_vector, p.work.ptr + 2 * per_vector, now, p.io.ptr, p.io_len.ptr, p.stream);
            LSR_HIP(hipMemcpyAsync(q + off, p.io.ptr, per_vector * 8, hipMemcpyDeviceToHost, p.stream));
            LSR_HIP(hipMemcpyAsync(len + done, p.io_len.ptr, now * sizeof(uint32_t), hipMemcpyDeviceToHost, p.stream));
        }
        LSR_HIP(hipStreamSynchronize(p.stream));
    }
}

// Split of an evaluation over slices (lsr_prove_kernels.hpp eval_slice_kernel) for `groups` = instances x point pairs polynomials
// of `len` coefficients: none up to 2^17 coefficients (the single-workgroup kernel, as before); above, slices of 16 .. 512 rows (doubling
// while that still leaves 2048 workgroups) and at most kEvalMaxSlices of them, so four instances at m = 2^20 run 1024 workgroups instead of 4.
constexpr uint32_t kEvalMaxSlices = 1024;
struct EvalSplit {
    uint32_t slices, rows;
};
static EvalSplit eval_split(size_t len, size_t groups) {
    if (len <= (size_t)kEvalPass) return {1u, 0u};
    const size_t rows = (len + kEvalBlock - 1) / kEvalBlock;
    size_t per = 16;
    while ((per < (size_t)kEvalRows && rows * groups / (2 * per) >= 2048) || (rows + per - 1) / per > kEvalMaxSlices) per *= 2;
    return {(uint32_t)((rows + per - 1) / per), (uint32_t)per};
}

template <bool BITREV, int NPOLY>
static void launch_eval(const EvalPolys& polys, const EvalPoints& pts, const EvalOut& out, int logm, uint64_t scale_mont, size_t count, uint32_t pairs,
                        uint32_t slices, uint32_t rows_per_slice, uint64_t* part, hipStream_t s) {
    if (slices <= 1) {
        hipLaunchKernelGGL((eval_kernel<BITREV, NPOLY>), dim3((unsigned)count, pairs), dim3(kEvalBlock), 0, s, polys, pts, out, logm, scale_mont);
        return;
    }
    hipLaunchKernelGGL((eval_slice_kernel<BITREV, NPOLY>), dim3((unsigned)count, pairs, slices), dim3(kEvalBlock), 0, s, polys, pts, part, logm,
                       rows_per_slice);
    const size_t lanes = count * pairs * (size_t)(NPOLY * 2);
    hipLaunchKernelGGL((eval_combine_kernel<NPOLY>), dim3(blocks_for(lanes, ~0u)), dim3(kBlock), 0, s, part, pairs, slices, pts.count, out, scale_mont, lanes);
}

// ---- prove_r1cs / prove_r1cs_zk for a batch (lib.rs:747-809, 877-980) ----------------------------------
// Per chunk, all on one stream: constraint evals (from device witnesses) -> quotient pass with A's and B's interpolants stashed ->
// message Q' mod commit_modulus -> keys -> rows -> alpha -> beta -> evaluations -> proof records.
static void ensure_prove_workspace(LsrR1csProver& r, size_t chunk, size_t n_public) {
    ensure_workspace(*r.plan, chunk, false);
    r.witness.reserve(chunk * r.n_vars);
    const size_t c = std::max(r.ws.chunk, chunk);
    r.stash.reserve(2 * c * r.m);
    r.quot.reserve(c * r.m);
    r.msg.reserve(c * (r.m + 1));
    r.len.reserve(c);
    if (r.m > (uint32_t)kEvalPass) r.eval_part.reserve(c * kEvalMaxSlices * 6);
    r.ws.grow(c, n_public);
}

// one chunk of `count` instances.  d_z [count][n_vars]; d_blind [count] (zk) or nullptr; outputs device arrays.  host_keys: derive the
// keys on the host (seed 0 = fresh entropy) from the messages copied back.
static void prove_chunk(LsrR1csProver& r, const R1csProveCall& a, const uint64_t* d_z, const uint64_t* d_blind, const uint64_t* seeds, size_t count,
                        uint64_t* d_rows, uint64_t* d_proofs, uint8_t* d_hashes, uint32_t* d_status, bool host_keys, hipStream_t s) {
    LsrQuotientPlan& p = *r.plan;
    const size_t per_vector = count << p.logm;
    const size_t words = lsr_lwe_commitment_words(a.lwe);
    const R1csSlots v = r.ws.slots();
    const CsrView ca{r.row_ptr[0].ptr, r.col[0].ptr, r.val[0].ptr}, cb{r.row_ptr[1].ptr, r.col[1].ptr, r.val[1].ptr},
        cc{r.row_ptr[2].ptr, r.col[2].ptr, r.val[2].ptr};
    uint64_t* work = p.work.ptr;
    hipLaunchKernelGGL(constraint_evals_kernel, dim3(blocks_for(per_vector), 3), dim3(kBlock), 0, s, work, ca, cb, cc, d_z, r.n_vars, p.logm, per_vector);
    LSR_HIP(hipGetLastError());
    quotient_pass(p, work, work + per_vector, work + 2 * per_vector, count, r.quot.ptr, r.len.ptr, s, r.stash.ptr);
    // commitment message: Q (plain) or Q' = Q + r (X^m - 1) (zk), mod commit_modulus
    const uint32_t msg_len = r.m + (d_blind ? 1u : 0u);
    hipLaunchKernelGGL(prove_message_kernel, dim3(blocks_for(count * msg_len)), dim3(kBlock), 0, s, r.quot.ptr, r.m, d_blind, a.commit_modulus, r.msg.ptr,
                       msg_len, count * (size_t)msg_len);
    LSR_HIP(hipGetLastError());
    commit_messages(a.lwe, r.msg.ptr, msg_len, count, seeds, v.keys, d_rows, host_keys, s);
    r1cs_transcript(gather_publics_kernel, v, d_z, r.n_vars, a.n_public, d_rows, words, count, kProverModulus, s);
    // A, B, C (stash, stash + per_vector, third plane: m P coeffs) and Q (natural order) at alpha and beta
    const EvalPoints pts{{v.alphas, v.betas}, 1, 2};
    const uint64_t m_inv = prover_montgomery(invmod_prime(r.m % kProverModulus, kProverModulus));
    const EvalPolys abc{{r.stash.ptr, r.stash.ptr + per_vector, work + 2 * per_vector}, r.m, r.m};
    const EvalSplit split = eval_split(r.m, count);
    launch_eval<true, 3>(abc, pts, EvalOut{v.ev, 8, 2}, p.logm, m_inv, count, 1, split.slices, split.rows, r.eval_part.ptr, s);
    const EvalPolys qp{{r.quot.ptr, r.quot.ptr, r.quot.ptr}, r.m, r.m};
    launch_eval<false, 1>(qp, pts, EvalOut{v.ev + 6, 8, 0}, p.logm, kGoldOneMont, count, 1, split.slices, split.rows, r.eval_part.ptr, s);
    hipLaunchKernelGGL(prove_assemble_kernel, dim3(blocks_for(count, ~0u)), dim3(kBlock), 0, s, v.ev, v.alphas, v.betas, d_blind, r.len.ptr, v.hash_a,
                       v.hash_b, p.logm, d_proofs, reinterpret_cast<uint64_t*>(d_hashes), d_status, count);
    LSR_HIP(hipGetLastError());
}

// device arrays on `s` (on_device) or host arrays through the plan's stream
static void prove(LsrR1csProver& r, const R1csProveCall& c, bool on_device, hipStream_t s) {
    LsrQuotientPlan& p = *r.plan;
    const R1csProverRef ref{p.device, p.mutex, p.ev_last, p.stream, r.witness, r.n_vars, r.ws};
    const auto grow = [&](size_t chunk) { ensure_prove_workspace(r, chunk, c.n_public); };
    const auto chunk = [&](auto... args) { prove_chunk(r, c, args...); };
    if (on_device) r1cs_prove_device(ref, c, quotient_chunk(p, c.batch), grow, chunk, s);
    else r1cs_prove_host(ref, c, quotient_chunk(p, c.batch), grow, chunk);
}

static void verify_host(uint32_t m, const uint64_t* pub, size_t n_public, const uint64_t* rows, size_t words, const uint64_t* proofs, size_t batch, bool zk,
                        int* results) {
    r1cs_verify_host(kProverModulus, pub, n_public, rows, words, proofs, batch, results,
                     [&](const uint64_t* proof, uint64_t alpha, uint64_t beta) { return verify_one(proof, alpha, beta, m, zk); });
}

static void verify_device(uint32_t m, const uint64_t* d_pub, size_t n_public, const uint64_t* d_rows, size_t words, const uint64_t* d_proofs, size_t batch,
                          bool zk, int* d_results, hipStream_t s) {
    r1cs_verify_device(kProverModulus, d_pub, n_public, d_rows, words, batch, s, [&](const uint64_t* d_alphas, const uint64_t* d_betas) {
        hipLaunchKernelGGL(verify_check_kernel, dim3(blocks_for(batch, ~0u)), dim3(kBlock), 0, s, d_proofs, d_alphas, d_betas, m, zk ? 1 : 0, d_results, batch);
    });
}

static void eval_device(const uint64_t* d_c, size_t len, size_t batch, const uint64_t* d_x, uint32_t ppp, uint64_t* d_v, hipStream_t s) {
    // Few long polynomials (fewer than 1024 workgroups of more than 2^17 coefficients): the rows are spread over slices (eval_split), with
    // the per-slice sums in stream-ordered scratch.  A capturing stream (no allocation inside a capture) keeps the one-workgroup walk.
    const uint32_t pairs = (ppp + 1) / 2;
    EvalSplit split{1u, 0u};
    if (batch * pairs < 1024 && !stream_is_capturing(s)) split = eval_split(len, batch * pairs);
    const uint32_t slices = split.slices, per_slice = split.rows;
    uint64_t* part = nullptr;
    if (slices > 1) LSR_HIP(hipMallocAsync(reinterpret_cast<void**>(&part), batch * pairs * slices * 2 * 8, s));
    try {
        for (size_t done = 0; done < batch; done += 0x7fffffffull) {   // grid.x bound (a sliced call has batch < 1024: one trip)
            const size_t now = std::min<size_t>(0x7fffffffull, batch - done);
            const uint64_t* c = d_c + done * len;
            const EvalPolys polys{{c, c, c}, len, (uint32_t)len};
            const EvalPoints pts{{d_x + done * ppp, d_x + done * ppp + 1}, ppp, ppp};
            launch_eval<false, 1>(polys, pts, EvalOut{d_v + done * ppp, ppp, 0}, 0, kGoldOneMont, now, pairs, slices, per_slice, part, s);
        }
        LSR_HIP(hipGetLastError());
    } catch (...) {
        if (part) (void)hipFreeAsync(part, s);
        throw;
    }
    if (part) LSR_HIP(hipFreeAsync(part, s));
}

// natural-order transforms for host callers: ntt.rs:117-201
static void cyclic_host(const NttContext& c, uint64_t* values, size_t batch, bool inverse) {
    DeviceGuard guard(c.device);
    const size_t n = c.degree;
    const size_t chunk = std::max<size_t>(1, std::min<size_t>(batch, (256ull << 20) / (n * 8)));
    DeviceBuffer<uint64_t> x(chunk * n), y(chunk * n);
    std::lock_guard<std::mutex> lock(c.staging_mutex);   // serialises use of work_stream(c)
    for (size_t done = 0; done < batch; done += chunk) {
        const size_t now = std::min(chunk, batch - done);
        LSR_HIP(hipMemcpyAsync(x.ptr, values + done * n, now * n * 8, hipMemcpyHostToDevice, work_stream(c)));
        if (inverse) {
            launch_bit_reverse(y.ptr, x.ptr, c.logn, now, work_stream(c));
            launch_ntt(c, y.ptr, now, true, work_stream(c));
        } else {
            launch_ntt(c, x.ptr, now, false, work_stream(c));
            launch_bit_reverse(y.ptr, x.ptr, c.logn, now, work_stream(c));
        }
        LSR_HIP(hipMemcpyAsync(values + done * n, y.ptr, now * n * 8, hipMemcpyDeviceToHost, work_stream(c)));
        LSR_HIP(hipStreamSynchronize(work_stream(c)));
    }
}

}  // namespace lsr

using lsr::set_last_error;

using lsr::abi_guarded;
using lsr::abi_refuse;

extern "C" {

uint64_t lsr_prover_modulus(void) noexcept { return lsr::kProverModulus; }
uint64_t lsr_prover_root_2_32(void) noexcept { return lsr::kProverRoot2_32; }
uint64_t lsr_prover_root_of_unity(uint64_t n) noexcept { return lsr::prover_root_of_unity(lsr::kProverModulus, n); }

NttContext* lsr_cyclic_ntt_context_create(uint64_t q, uint32_t n, uint64_t omega, int device) noexcept {
    try {
        return lsr::create_cyclic_ntt_context(q, n, omega, device);
    } catch (...) {
        return nullptr;
    }
}
NttContext* lsr_cyclic_ntt_context_create_large(uint64_t q, uint32_t n, uint64_t omega, int device) noexcept {
    try {
        return lsr::create_cyclic_ntt_context(q, n, omega, device, true, "lsr_cyclic_ntt_context_create_large");
    } catch (...) {
        return nullptr;
    }
}
uint32_t lsr_prover_max_log2_size(void) noexcept { return lsr::kProverMaxLog2; }
int lsr_ntt_context_is_cyclic(const NttContext* ctx) noexcept { return ctx && ctx->cyclic ? 1 : 0; }

int lsr_cyclic_ntt_forward_batch(const NttContext* ctx, uint64_t* values, size_t batch) noexcept {
    if (lsr::refuse_coeff_context("lsr_cyclic_ntt_forward_batch", ctx)) return -1;
    if (!ctx || !values || !ctx->cyclic) return -1;
    if (batch == 0) return 0;
    return abi_guarded("lsr_cyclic_ntt_forward_batch", [&] { lsr::cyclic_host(*ctx, values, batch, false); });
}
int lsr_cyclic_ntt_inverse_batch(const NttContext* ctx, uint64_t* values, size_t batch) noexcept {
    if (lsr::refuse_coeff_context("lsr_cyclic_ntt_inverse_batch", ctx)) return -1;
    if (!ctx || !values || !ctx->cyclic) return -1;
    if (batch == 0) return 0;
    return abi_guarded("lsr_cyclic_ntt_inverse_batch", [&] { lsr::cyclic_host(*ctx, values, batch, true); });
}
int lsr_bit_reverse_device(uint64_t* d_out, const uint64_t* d_in, int logn, size_t batch, void* stream) noexcept {
    if (!d_out || !d_in || d_out == d_in || logn < 1 || logn > 31) return -1;
    return abi_guarded("lsr_bit_reverse_device", [&] { lsr::launch_bit_reverse(d_out, d_in, logn, batch, static_cast<hipStream_t>(stream)); });
}

LsrQuotientPlan* lsr_quotient_plan_create(uint32_t m, int device) noexcept {
    try {
        return lsr::create_plan(m, device, false, "lsr_quotient_plan_create");
    } catch (...) {
        return nullptr;
    }
}
LsrQuotientPlan* lsr_quotient_plan_create_large(uint32_t m, int device) noexcept {
    try {
        return lsr::create_plan(m, device, true, "lsr_quotient_plan_create_large");
    } catch (...) {
        return nullptr;
    }
}
void lsr_quotient_plan_free(LsrQuotientPlan* plan) noexcept { lsr::destroy_plan(plan); }
uint32_t lsr_quotient_plan_size(const LsrQuotientPlan* plan) noexcept { return plan ? plan->m : 0; }

int lsr_quotient_batch(LsrQuotientPlan* plan, const uint64_t* a_evals, const uint64_t* b_evals, const uint64_t* c_evals, size_t batch,
                       uint64_t* quotient, uint32_t* quotient_len) noexcept {
    if (!plan || !a_evals || !b_evals || !c_evals || !quotient || !quotient_len) return -1;
    if (batch == 0) return 0;
    return abi_guarded("lsr_quotient_batch", [&] { lsr::quotient_host(*plan, a_evals, b_evals, c_evals, batch, quotient, quotient_len); });
}
int lsr_quotient_batch_device(LsrQuotientPlan* plan, const uint64_t* d_a, const uint64_t* d_b, const uint64_t* d_c, size_t batch, uint64_t* d_quotient,
                              uint32_t* d_quotient_len, void* stream) noexcept {
    if (!plan || !d_a || !d_b || !d_c || !d_quotient || !d_quotient_len) return -1;
    if (batch == 0) return 0;
    return abi_guarded("lsr_quotient_batch_device",
                   [&] { lsr::quotient_device(*plan, d_a, d_b, d_c, batch, d_quotient, d_quotient_len, static_cast<hipStream_t>(stream)); });
}

LsrR1csProver* lsr_r1cs_prover_create(const SparseMatrix* A, const SparseMatrix* B, const SparseMatrix* C, int device) noexcept {
    if (!A || !B || !C) return nullptr;
    try {
        const SparseMatrix* const mats[3] = {A, B, C};
        return lsr::create_prover(mats, device);
    } catch (...) {
        return nullptr;
    }
}
void lsr_r1cs_prover_free(LsrR1csProver* prover) noexcept { lsr::destroy_prover(prover); }
uint32_t lsr_r1cs_prover_num_constraints(const LsrR1csProver* prover) noexcept { return prover ? prover->m : 0; }
uint32_t lsr_r1cs_prover_num_variables(const LsrR1csProver* prover) noexcept { return prover ? prover->n_vars : 0; }

int lsr_r1cs_constraint_evals_batch(LsrR1csProver* prover, const uint64_t* witnesses, size_t batch, uint64_t* a_evals, uint64_t* b_evals,
                                    uint64_t* c_evals) noexcept {
    if (!prover || !witnesses || !a_evals || !b_evals || !c_evals) return -1;
    if (batch == 0) return 0;
    return abi_guarded("lsr_r1cs_constraint_evals_batch", [&] {
        uint64_t* const evals[3] = {a_evals, b_evals, c_evals};
        if (prover->lag) lsr::lagrange_host_run(*prover->lag, witnesses, batch, evals, nullptr, nullptr, nullptr);
        else lsr::prover_run(*prover, witnesses, batch, evals, nullptr, nullptr);
    });
}
int lsr_r1cs_quotient_batch(LsrR1csProver* prover, const uint64_t* witnesses, size_t batch, uint64_t* quotient, uint32_t* quotient_len) noexcept {
    if (!prover || !witnesses || !quotient || !quotient_len) return -1;
    if (batch == 0) return 0;
    return abi_guarded("lsr_r1cs_quotient_batch", [&] {
        if (prover->lag) lsr::lagrange_host_run(*prover->lag, witnesses, batch, nullptr, nullptr, quotient, quotient_len);
        else lsr::prover_run(*prover, witnesses, batch, nullptr, quotient, quotient_len);
    });
}

// ---- batched prove / verify (prover.h) ----
static int prove_checks(const char* where, const LsrR1csProver* prover, const LweContext* lwe, uint64_t commit_modulus, const void* w, size_t n_public,
                        const uint64_t* seeds, const void* rows, const void* proofs, const void* status) {
    if (!prover || !lwe) return abi_refuse(where, "NULL prover or LWE context");
    if (!w || !seeds || !rows || !proofs || !status) return abi_refuse(where, "NULL witnesses, seeds, rows, proofs or status");
    if (n_public > prover->n_vars) return abi_refuse(where, "n_public exceeds the circuit's variable count");
    if (commit_modulus <= 1) return abi_refuse(where, "commit_modulus must be LweContext::modulus() (> 1)");
    if (lsr::refuse_rns_context(where, lwe)) return -1;
    const NttContext* ntt = lsr_lwe_ntt_context(lwe);
    if (!ntt || ntt->device != prover->device()) return abi_refuse(where, "the prover and the LWE context live on different devices");
    return 0;
}

int lsr_r1cs_prove_batch(LsrR1csProver* prover, LweContext* lwe, uint64_t commit_modulus, const uint64_t* witnesses, size_t batch, size_t n_public,
                         const uint64_t* seeds, const uint64_t* blinding, uint64_t* rows, uint64_t* proofs, uint8_t* hashes, uint32_t* status) noexcept {
    const char* where = "lsr_r1cs_prove_batch";
    if (prove_checks(where, prover, lwe, commit_modulus, witnesses, n_public, seeds, rows, proofs, status)) return -1;
    if (batch == 0) return 0;
    const lsr::R1csProveCall c{lwe, commit_modulus, n_public, seeds, witnesses, blinding, rows, proofs, hashes, status, batch};
    return abi_guarded(where, [&] {
        if (prover->lag) lsr::lagrange_prove(*prover->lag, c, false, nullptr);
        else lsr::prove(*prover, c, false, nullptr);
    });
}

int lsr_r1cs_prove_batch_device(LsrR1csProver* prover, LweContext* lwe, uint64_t commit_modulus, const uint64_t* d_witnesses, size_t batch, size_t n_public,
                                const uint64_t* seeds, const uint64_t* d_blinding, uint64_t* d_rows, uint64_t* d_proofs, uint8_t* d_hashes, uint32_t* d_status,
                                void* stream) noexcept {
    const char* where = "lsr_r1cs_prove_batch_device";
    if (prove_checks(where, prover, lwe, commit_modulus, d_witnesses, n_public, seeds, d_rows, d_proofs, d_status)) return -1;
    if (batch == 0) return 0;
    const lsr::R1csProveCall c{lwe, commit_modulus, n_public, seeds, d_witnesses, d_blinding, d_rows, d_proofs, d_hashes, d_status, batch};
    return lsr::abi_prove_device(where, "lsr_r1cs_prove_batch", seeds, batch, prover->device(), stream, [&](hipStream_t s) {
        if (prover->lag) lsr::lagrange_prove(*prover->lag, c, true, s);
        else lsr::prove(*prover, c, true, s);
    });
}

static int verify_checks(const char* where, uint32_t m, const void* pub, size_t n_public, const void* rows, size_t words, const void* proofs,
                         const void* results) {
    if ((!pub && n_public) || !rows || !proofs || !results) return abi_refuse(where, "NULL public inputs, rows, proofs or results");
    if (words == 0) return abi_refuse(where, "words_per_row must be positive");
    if (m == 0 || (m & (m - 1))) return abi_refuse(where, "m must be a power of two (the NTT path, r1cs.rs:386-389)");
    return 0;
}

int lsr_r1cs_verify_batch(uint32_t m, const uint64_t* public_inputs, size_t n_public, const uint64_t* rows, size_t words_per_row, const uint64_t* proofs,
                          size_t batch, int zk, int* results) noexcept {
    const char* where = "lsr_r1cs_verify_batch";
    if (verify_checks(where, m, public_inputs, n_public, rows, words_per_row, proofs, results)) return -1;
    if (batch == 0) return 0;
    return abi_guarded(where, [&] { lsr::verify_host(m, public_inputs, n_public, rows, words_per_row, proofs, batch, zk != 0, results); });
}

int lsr_r1cs_verify_batch_device(uint32_t m, const uint64_t* d_public_inputs, size_t n_public, const uint64_t* d_rows, size_t words_per_row,
                                 const uint64_t* d_proofs, size_t batch, int zk, int* d_results, void* stream) noexcept {
    const char* where = "lsr_r1cs_verify_batch_device";
    if (verify_checks(where, m, d_public_inputs, n_public, d_rows, words_per_row, d_proofs, d_results)) return -1;
    if (batch == 0) return 0;
    return abi_guarded(where, [&] {
        lsr::verify_device(m, d_public_inputs, n_public, d_rows, words_per_row, d_proofs, batch, zk != 0, d_results, static_cast<hipStream_t>(stream));
    });
}

int lsr_prover_eval_batch_device(const uint64_t* d_coeffs, size_t len, size_t batch, const uint64_t* d_points, uint32_t points_per_poly, uint64_t* d_values,
                                 void* stream) noexcept {
    const char* where = "lsr_prover_eval_batch_device";
    if (!d_coeffs || !d_points || !d_values) return abi_refuse(where, "NULL coefficients, points or values");
    if (len == 0 || len > 0x80000000ull) return abi_refuse(where, "len must be in [1, 2^31]");
    if (points_per_poly == 0 || points_per_poly > 131070u) return abi_refuse(where, "points_per_poly must be in [1, 131070]");
    if (batch == 0) return 0;
    return abi_guarded(where, [&] { lsr::eval_device(d_coeffs, len, batch, d_points, points_per_poly, d_values, static_cast<hipStream_t>(stream)); });
}

// ---- the Lagrange path (prover.h) ----
LsrR1csProver* lsr_r1cs_prover_create_mod(const SparseMatrix* A, const SparseMatrix* B, const SparseMatrix* C, uint64_t modulus, int device) noexcept {
    if (!A || !B || !C) {
        set_last_error("lsr_r1cs_prover_create_mod: NULL matrix");
        return nullptr;
    }
    const uint32_t m = A->n_rows;
    if (modulus == lsr::kProverModulus && m != 0 && (m & (m - 1)) == 0) return lsr_r1cs_prover_create(A, B, C, device);   // should_use_ntt
    try {
        const SparseMatrix* const mats[3] = {A, B, C};
        lsr::LagrangeProverPtr lag(lsr::lagrange_create(mats, modulus, device));
        if (!lag) return nullptr;
        auto* r = new LsrR1csProver;
        r->m = m;
        r->n_vars = A->n_cols;
        r->lag = std::move(lag);
        r->modulus = modulus;
        return r;
    } catch (...) {
        set_last_error("lsr_r1cs_prover_create_mod: allocation failed");
        return nullptr;
    }
}
uint64_t lsr_r1cs_prover_modulus(const LsrR1csProver* prover) noexcept { return prover ? prover->modulus : 0; }
int lsr_r1cs_prover_uses_ntt(const LsrR1csProver* prover) noexcept { return prover && prover->plan ? 1 : 0; }

int lsr_r1cs_interpolate_batch(LsrR1csProver* prover, const uint64_t* witnesses, size_t batch, uint64_t* a_coeffs, uint64_t* b_coeffs,
                               uint64_t* c_coeffs) noexcept {
    const char* where = "lsr_r1cs_interpolate_batch";
    if (!prover || !witnesses || !a_coeffs || !b_coeffs || !c_coeffs) return abi_refuse(where, "NULL prover, witnesses or output");
    if (!prover->lag) return abi_refuse(where, "only a Lagrange-path prover (lsr_r1cs_prover_uses_ntt == 0) exposes its interpolants");
    if (batch == 0) return 0;
    return abi_guarded(where, [&] {
        uint64_t* const out[3] = {a_coeffs, b_coeffs, c_coeffs};
        lsr::lagrange_host_run(*prover->lag, witnesses, batch, nullptr, out, nullptr, nullptr);
    });
}

static bool ntt_path(uint32_t m, uint64_t q) { return q == lsr::kProverModulus && (m & (m - 1)) == 0; }

static int verify_mod_checks(const char* where, uint32_t m, uint64_t q, const void* pub, size_t n_public, const void* rows, size_t words,
                             const void* proofs, const void* results) {
    if ((!pub && n_public) || !rows || !proofs || !results) return abi_refuse(where, "NULL public inputs, rows, proofs or results");
    if (words == 0) return abi_refuse(where, "words_per_row must be positive");
    if (q < 3 || (q & 1) == 0) return abi_refuse(where, "the modulus must be odd and >= 3");
    if (m == 0) return abi_refuse(where, "m must be positive");
    if (!ntt_path(m, q) && m > lsr::kLagrangeMaxM) return abi_refuse(where, "the Lagrange path takes m <= 8192");
    return 0;
}

int lsr_r1cs_verify_batch_mod(uint32_t m, uint64_t modulus, const uint64_t* public_inputs, size_t n_public, const uint64_t* rows, size_t words_per_row,
                              const uint64_t* proofs, size_t batch, int zk, int* results) noexcept {
    const char* where = "lsr_r1cs_verify_batch_mod";
    if (verify_mod_checks(where, m, modulus, public_inputs, n_public, rows, words_per_row, proofs, results)) return -1;
    if (ntt_path(m, modulus)) return lsr_r1cs_verify_batch(m, public_inputs, n_public, rows, words_per_row, proofs, batch, zk, results);
    if (batch == 0) return 0;
    return abi_guarded(where, [&] { lsr::verify_mod_host(m, modulus, public_inputs, n_public, rows, words_per_row, proofs, batch, zk != 0, results); });
}

int lsr_r1cs_verify_batch_mod_device(uint32_t m, uint64_t modulus, const uint64_t* d_public_inputs, size_t n_public, const uint64_t* d_rows,
                                     size_t words_per_row, const uint64_t* d_proofs, size_t batch, int zk, int* d_results, void* stream) noexcept {
    const char* where = "lsr_r1cs_verify_batch_mod_device";
    if (verify_mod_checks(where, m, modulus, d_public_inputs, n_public, d_rows, words_per_row, d_proofs, d_results)) return -1;
    if (ntt_path(m, modulus))
        return lsr_r1cs_verify_batch_device(m, d_public_inputs, n_public, d_rows, words_per_row, d_proofs, batch, zk, d_results, stream);
    if (batch == 0) return 0;
    return abi_guarded(where, [&] {
        lsr::verify_mod_device(m, modulus, d_public_inputs, n_public, d_rows, words_per_row, d_proofs, batch, zk != 0, d_results, static_cast<hipStream_t>(stream));
    });
}

}  // extern "C"
