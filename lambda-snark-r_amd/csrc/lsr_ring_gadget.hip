// Gadget decomposition for the module-SIS path (batch.h "gadget decomposition"): a ring element's coefficients written
// in D balanced base-2^b digits, the gadget product back, the l-infinity norm a verifier checks, and the commitment y = M G^-1(x) as
// ONE launch of the mat-vec's tile kernel with the digits extracted in its load stage (n <= 4096), so that the decomposed vector — D
// times the witness — never exists in memory.  Decompose, recompose and the norm are streaming kernels without a workspace.
#include <algorithm>

#include "lambda_snark/batch.h"
#include "lsr_flavour.hpp"
#include "lsr_ring_call.hpp"
#include "lsr_ring_gadget_kernels.hpp"
#include "lsr_ring_matrix.hpp"
#include "lsr_runtime.hpp"

namespace lsr {

static_assert(kGadgetMaxDigits == 64 / 2 + 1, "recompose takes b (D - 1) <= 64 with b >= 2");

// (gadget_admissible and gadget_params: lsr_ring_gadget_digits.hpp, shared with lsr_ring_mod_matvec.hip)

static unsigned stream_grid(size_t total) { return static_cast<unsigned>(std::min<size_t>((total + kThreads - 1) / kThreads, 256 * 32)); }

static void decompose_device(const NttContext& c, uint64_t* d_out, const uint64_t* d_x, size_t count, unsigned b, uint64_t digits, hipStream_t s) {
    const size_t total = count << c.logn;
    hipLaunchKernelGGL(ring_decompose_kernel, dim3(stream_grid(total)), dim3(kThreads), 0, s, d_out, d_x, total, c.logn, c.modulus, gadget_params(c.modulus, b, digits));
    LSR_HIP(hipGetLastError());
}

static void recompose_device(const NttContext& c, uint64_t* d_out, const uint64_t* d_z, size_t count, unsigned b, uint64_t digits, hipStream_t s) {
    GadgetPowers w{};
    const uint64_t base = (uint64_t)(((u128)1 << b) % c.modulus);
    uint64_t pw = 1 % c.modulus;
    for (uint64_t d = 0; d < digits; ++d, pw = mulmod(pw, base, c.modulus)) w.pw[d] = pw;
    const size_t total = count << c.logn;
    const dim3 grid(stream_grid(total));
    if (c.gold) hipLaunchKernelGGL(ring_recompose_kernel<true>, grid, dim3(kThreads), 0, s, d_out, d_z, total, c.logn, (uint32_t)digits, c.mod, w);
    else hipLaunchKernelGGL(ring_recompose_kernel<false>, grid, dim3(kThreads), 0, s, d_out, d_z, total, c.logn, (uint32_t)digits, c.mod, w);
    LSR_HIP(hipGetLastError());
}

static void linf_device(const NttContext& c, const uint64_t* d_x, size_t count, uint64_t* d_linf, hipStream_t s) {
    const unsigned threads = std::min<unsigned>(std::max<unsigned>(c.degree, 64), kThreads);
    const unsigned grid = static_cast<unsigned>(std::min<size_t>(count, 1u << 20));
    hipLaunchKernelGGL(ring_linf_kernel, dim3(grid), dim3(threads), 0, s, d_linf, d_x, count, c.logn, c.modulus);
    LSR_HIP(hipGetLastError());
}

template <class A, int LT>
static void gadget_tile(const LsrRingMatrix& m, uint64_t* d_y, const uint64_t* d_x, size_t batch, const GadgetParams& g, hipStream_t s) {
    const NttContext& c = *m.ctx;
    constexpr int RB = MatvecRowBlock<A>::value;
    const size_t total = batch << c.logn;
    const dim3 grid(static_cast<unsigned>((total + kTile - 1) / kTile), static_cast<unsigned>((m.rows + RB - 1) / RB));
    hipLaunchKernelGGL((ntt_tile_ring_matvec_gadget<A, LT, RB>), grid, dim3(kThreads), 0, s, d_y, d_x, m.data.ptr, total, (uint32_t)m.rows,
                       (uint32_t)(m.cols / g.digits), g, c.mod, Flavour<A>::fwd(c), Flavour<A>::inv(c), Flavour<A>::consts(c));
}

template <class A>
static void gadget_tile_lt(const LsrRingMatrix& m, uint64_t* d_y, const uint64_t* d_x, size_t batch, const GadgetParams& g, hipStream_t s) {
    for_tile_log<1, 12>(m.ctx->logn, [&](auto t) { gadget_tile<A, decltype(t)::value>(m, d_y, d_x, batch, g, s); });
}

// n <= 4096 (caller validated the arguments)
static void matvec_gadget_device(const LsrRingMatrix& m, uint64_t* d_y, const uint64_t* d_x, size_t batch, unsigned b, uint64_t digits, hipStream_t s) {
    const NttContext& c = *m.ctx;
    const GadgetParams g = gadget_params(c.modulus, b, digits);
    if (!stream_is_capturing(s)) m.ready.wait(s);
    for_flavour(c, [&](auto a) { gadget_tile_lt<decltype(a)>(m, d_y, d_x, batch, g, s); });
    LSR_HIP(hipGetLastError());
}

// (host buffers: host_staged, lsr_ring_call.hpp)

}  // namespace lsr

// ------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------
// The refusals of batch.h, in its order.  Steps 1 and 2 read neither handle; step 3 reads the context's modulus.
static int shape_check(const char* where, unsigned b, size_t digits, bool recompose) {
    if (b < 2 || b > 32) return lsr::abi_refuse(where, "base_log2 = " + std::to_string(b) + " is outside [2, 32]");
    if (digits == 0) return lsr::abi_refuse(where, "digits must be at least 1");
    if (recompose ? digits - 1 > 64 / b : digits > 64 / b)
        return lsr::abi_refuse(where, std::string(recompose ? "base_log2 * (digits - 1)" : "base_log2 * digits") + " is above 64 (base_log2 = " +
                                          std::to_string(b) + ", digits = " + std::to_string(digits) + ")");
    return 0;
}

static int admissible_check(const char* where, const NttContext& ctx, unsigned b, size_t digits) {
    if (lsr::gadget_admissible(ctx.modulus, b, digits)) return 0;
    const uint64_t need = lsr_ring_gadget_min_digits(ctx.modulus, b);
    return lsr::abi_refuse(where, "(base_log2 = " + std::to_string(b) + ", digits = " + std::to_string(digits) + ") is not admissible for q = " +
                                      std::to_string(ctx.modulus) +
                                      (need ? ": the digits do not cover the centred residues; lsr_ring_gadget_min_digits gives " + std::to_string(need)
                                            : ": no digit count is admissible at this base (lsr_ring_gadget_min_digits gives 0)"));
}

// every call here has one operand: `what` names the pair
static void require_apart(const void* out, size_t out_bytes, const void* in, size_t in_bytes, const char* what) {
    lsr::require_apart(out, out_bytes, in, in_bytes, (std::string(what) + ": the output must not share memory with the operand").c_str());
}

static int decompose_call(const char* where, const NttContext* ctx, uint64_t* out, const uint64_t* x, size_t count, unsigned b, size_t digits, bool device,
                          void* stream) noexcept {
    if (!ctx || !out || !x) return lsr::abi_refuse(where, "NULL context or buffer");
    if (shape_check(where, b, digits, false) != 0 || admissible_check(where, *ctx, b, digits) != 0) return -1;
    if (count == 0) return 0;
    return lsr::abi_guarded(where, [&] {
        const size_t n = ctx->degree;
        require_apart(out, count * digits * n * 8, x, count * n * 8, "out overlaps x");
        lsr::require_device();
        if (device) {
            lsr::DeviceGuard guard(ctx->device);
            lsr::decompose_device(*ctx, out, x, count, b, digits, static_cast<hipStream_t>(stream));
        } else {
            lsr::host_staged(*ctx, out, x, count, digits * n, n, [&](uint64_t* d_out, const uint64_t* d_in, size_t now, hipStream_t s) {
                lsr::decompose_device(*ctx, d_out, d_in, now, b, digits, s);
            });
        }
    });
}

static int recompose_call(const char* where, const NttContext* ctx, uint64_t* out, const uint64_t* z, size_t count, unsigned b, size_t digits, bool device,
                          void* stream) noexcept {
    if (!ctx || !out || !z) return lsr::abi_refuse(where, "NULL context or buffer");
    if (shape_check(where, b, digits, true) != 0) return -1;
    if (count == 0) return 0;
    return lsr::abi_guarded(where, [&] {
        const size_t n = ctx->degree;
        require_apart(out, count * n * 8, z, count * digits * n * 8, "out overlaps z");
        lsr::require_device();
        if (device) {
            lsr::DeviceGuard guard(ctx->device);
            lsr::recompose_device(*ctx, out, z, count, b, digits, static_cast<hipStream_t>(stream));
        } else {
            lsr::host_staged(*ctx, out, z, count, n, digits * n, [&](uint64_t* d_out, const uint64_t* d_in, size_t now, hipStream_t s) {
                lsr::recompose_device(*ctx, d_out, d_in, now, b, digits, s);
            });
        }
    });
}

static int linf_call(const char* where, const NttContext* ctx, const uint64_t* x, size_t count, uint64_t* linf, bool device, void* stream) noexcept {
    if (!ctx || !x || !linf) return lsr::abi_refuse(where, "NULL context or buffer");
    if (count == 0) return 0;
    return lsr::abi_guarded(where, [&] {
        const size_t n = ctx->degree;
        require_apart(linf, count * 8, x, count * n * 8, "linf overlaps x");
        lsr::require_device();
        if (device) {
            lsr::DeviceGuard guard(ctx->device);
            lsr::linf_device(*ctx, x, count, linf, static_cast<hipStream_t>(stream));
        } else {
            lsr::host_staged(*ctx, linf, x, count, 1, n, [&](uint64_t* d_out, const uint64_t* d_in, size_t now, hipStream_t s) {
                lsr::linf_device(*ctx, d_in, now, d_out, s);
            });
        }
    });
}

static int matvec_gadget_call(const char* where, const LsrRingMatrix* mat, uint64_t* y, const uint64_t* x, size_t batch, unsigned b, size_t digits,
                              bool device, void* stream) noexcept {
    if (!mat || !y || !x) return lsr::abi_refuse(where, "NULL matrix or buffer");
    if (shape_check(where, b, digits, false) != 0 || admissible_check(where, *mat->ctx, b, digits) != 0) return -1;
    if (mat->cols % digits != 0)
        return lsr::abi_refuse(where, "cols = " + std::to_string(mat->cols) + " of the matrix is not a multiple of digits = " + std::to_string(digits));
    if (batch == 0) return 0;
    return lsr::abi_guarded(where, [&] {
        const NttContext& ctx = *mat->ctx;
        const size_t n = ctx.degree, xcols = mat->cols / digits;
        require_apart(y, batch * mat->rows * n * 8, x, batch * xcols * n * 8, "y overlaps x");
        if (ctx.logn > lsr::kTileLog)
            throw std::runtime_error("n = " + std::to_string(n) + " is above 4096, where the product has no fused form: decompose x with "
                                     "lsr_ntt_ring_decompose_batch_device and pass the digits to lsr_ntt_ring_matvec_batch_device");
        lsr::require_device();
        if (device) {
            lsr::DeviceGuard guard(ctx.device);
            lsr::matvec_gadget_device(*mat, y, x, batch, b, digits, static_cast<hipStream_t>(stream));
        } else {
            lsr::host_staged(ctx, y, x, batch, mat->rows * n, xcols * n, [&](uint64_t* d_out, const uint64_t* d_in, size_t now, hipStream_t s) {
                lsr::matvec_gadget_device(*mat, d_out, d_in, now, b, digits, s);
            });
        }
    });
}

extern "C" {

uint64_t lsr_ring_gadget_min_digits(uint64_t q, unsigned base_log2) noexcept {
    if (base_log2 < 2 || base_log2 > 32) return 0;
    for (uint64_t digits = 1; digits <= 64 / base_log2; ++digits)
        if (lsr::gadget_admissible(q, base_log2, digits)) return digits;
    return 0;
}

int lsr_ntt_ring_decompose_batch(const NttContext* ctx, uint64_t* out, const uint64_t* x, size_t count, unsigned base_log2, size_t digits) noexcept {
    return decompose_call("lsr_ntt_ring_decompose_batch", ctx, out, x, count, base_log2, digits, false, nullptr);
}
int lsr_ntt_ring_decompose_batch_device(const NttContext* ctx, uint64_t* d_out, const uint64_t* d_x, size_t count, unsigned base_log2, size_t digits,
                                        void* stream) noexcept {
    return decompose_call("lsr_ntt_ring_decompose_batch_device", ctx, d_out, d_x, count, base_log2, digits, true, stream);
}

int lsr_ntt_ring_recompose_batch(const NttContext* ctx, uint64_t* out, const uint64_t* z, size_t count, unsigned base_log2, size_t digits) noexcept {
    return recompose_call("lsr_ntt_ring_recompose_batch", ctx, out, z, count, base_log2, digits, false, nullptr);
}
int lsr_ntt_ring_recompose_batch_device(const NttContext* ctx, uint64_t* d_out, const uint64_t* d_z, size_t count, unsigned base_log2, size_t digits,
                                        void* stream) noexcept {
    return recompose_call("lsr_ntt_ring_recompose_batch_device", ctx, d_out, d_z, count, base_log2, digits, true, stream);
}

int lsr_ntt_ring_linf_batch(const NttContext* ctx, const uint64_t* x, size_t count, uint64_t* linf) noexcept {
    return linf_call("lsr_ntt_ring_linf_batch", ctx, x, count, linf, false, nullptr);
}
int lsr_ntt_ring_linf_batch_device(const NttContext* ctx, const uint64_t* d_x, size_t count, uint64_t* d_linf, void* stream) noexcept {
    return linf_call("lsr_ntt_ring_linf_batch_device", ctx, d_x, count, d_linf, true, stream);
}

int lsr_ntt_ring_matvec_gadget_batch(const LsrRingMatrix* mat, uint64_t* y, const uint64_t* x, size_t batch, unsigned base_log2, size_t digits) noexcept {
    return matvec_gadget_call("lsr_ntt_ring_matvec_gadget_batch", mat, y, x, batch, base_log2, digits, false, nullptr);
}
int lsr_ntt_ring_matvec_gadget_batch_device(const LsrRingMatrix* mat, uint64_t* d_y, const uint64_t* d_x, size_t batch, unsigned base_log2, size_t digits,
                                            void* stream) noexcept {
    return matvec_gadget_call("lsr_ntt_ring_matvec_gadget_batch_device", mat, d_y, d_x, batch, base_log2, digits, true, stream);
}

}  // extern "C"
