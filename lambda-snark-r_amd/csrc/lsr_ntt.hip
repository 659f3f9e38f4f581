// NTT contexts, kernel dispatch and the ntt_* C-ABI (reference: cpp-core/src/ntt.cpp).
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <new>
#include <thread>
#include <type_traits>

#include "lambda_snark/batch.h"
#include "lambda_snark/ntt.h"
#include "lsr_flavour.hpp"
#include "lsr_ntt_kernels.hpp"
#include "lsr_runtime.hpp"

namespace lsr {

// ------------------------------------------------------------------------------------------------
// runtime plumbing
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_last_error;
void set_last_error(const std::string& msg) { g_last_error = msg; }
const char* last_error_cstr() { return g_last_error.c_str(); }

static std::atomic<int> g_arith_mode{0};
int arith_mode() { return g_arith_mode.load(); }

int visible_device_count() {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) return 0;
    return count;
}

// LAMBDA_SNARK_DEVICE, else LOCAL_RANK, else 0.  An index the process cannot see is an ERROR (-1), not wrapped around: a rank
// launched with more ranks than visible devices would otherwise silently share a GPU with another rank (round-2 verdict).
int default_device() {
    const int count = visible_device_count();
    if (count <= 0) return 0;
    for (const char* name : {"LAMBDA_SNARK_DEVICE", "LOCAL_RANK"}) {
        const char* s = std::getenv(name);
        if (!s || !*s) continue;
        char* end = nullptr;
        const long v = std::strtol(s, &end, 10);
        if (*end != 0 || v < 0 || v >= count) {
            set_last_error(std::string(name) + "=" + s + " does not name one of the " + std::to_string(count) + " visible HIP devices");
            std::fprintf(stderr, "lambda_snark_core: %s=%s does not name one of the %d visible HIP devices\n", name, s, count);
            return -1;
        }
        return static_cast<int>(v);
    }
    return 0;
}

bool stream_is_capturing(hipStream_t stream) {
    hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &status) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return status != hipStreamCaptureStatusNone;
}

__global__ void __launch_bounds__(256) zero_words_kernel(uint64_t* __restrict__ dst, size_t words) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < words; i += stride) dst[i] = 0;
}
void zero_words_async(uint64_t* dst, size_t words, hipStream_t stream) {
    if (!words) return;
    const unsigned grid = static_cast<unsigned>(std::min<size_t>((words + 255) / 256, 4096));
    hipLaunchKernelGGL(zero_words_kernel, dim3(grid), dim3(256), 0, stream, dst, words);
    LSR_HIP(hipGetLastError());
}

DeviceGuard::DeviceGuard(int device) {
    if (hipGetDevice(&previous_) != hipSuccess) previous_ = -1;
    if (previous_ != device) {
        LSR_HIP(hipSetDevice(device));
        switched_ = true;
    }
}
DeviceGuard::~DeviceGuard() {
    if (switched_ && previous_ >= 0) (void)hipSetDevice(previous_);
}

// ------------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------------
int resolve_device(const char* where, int device, bool announce) {
    const int devices = visible_device_count();
    if (devices <= 0) {
        set_last_error(std::string(where) + ": no HIP device visible — this library has no CPU fallback");
        if (announce) std::fprintf(stderr, "lambda_snark_core: no HIP device visible; the MI355X backend has no CPU fallback\n");
        return -1;
    }
    if (device < 0) return default_device();                 // -1 with its message when that names no visible device
    if (device >= devices) {
        set_last_error(std::string(where) + ": device index out of range");
        return -1;
    }
    return device;
}

// Whether run_ntt's two-pass FP64 transform may hand its intermediate over in 6 bytes per residue (lsr_arith.hpp pack48_from_f64): the
// forward hand-off is bounded by q + r_top * 0.875 q, the re-centred inverse one by 2 q, and both must stay below 2^47, i.e.
// (8 + 7 r_top) q < 2^50 — q < 2^47 / 4.5 for the four-stage round of n <= 2^16, q < 2^47 / 5.375 for the five stages of n = 2^17.
// LAMBDA_SNARK_NTT_HANDOFF=8, read when the context is created, keeps the 8-byte hand-off.
static bool handoff_is_packed(uint64_t q, int logn, bool use_f64) {
    if (!use_f64 || logn <= kTileLog || logn > kTwoPassMaxLog2) return false;
    if (const char* e = std::getenv("LAMBDA_SNARK_NTT_HANDOFF")) {
        if (std::strcmp(e, "8") == 0) return false;
    }
    const uint64_t r_top = static_cast<uint64_t>(std::max(logn - kTileLog, 4));
    return static_cast<u128>(q) * (8 + 7 * r_top) < (static_cast<u128>(1) << 50);
}

static NttContext* build_context(const char* where, uint64_t q, uint32_t n, int logn, int device, const TwiddleTables& tw, bool cyclic) {
    device = resolve_device(where, device, true);
    if (device < 0) return nullptr;
    NttContextPtr ctx(new NttContext);
    try {
        DeviceGuard guard(device);
        ctx->modulus = q;
        ctx->degree = n;
        ctx->logn = logn;
        ctx->device = device;
        ctx->psi = tw.psi;
        ctx->cyclic = cyclic;
        ctx->coeff = tw.fwd.empty();   // no tables: a ring handle's coefficient context (create_coeff_context), any q >= 2 below 2^45
        ctx->gold = !ctx->coeff && (q == kProverModulus);
        ctx->mod = make_mod_params(q, logn);
        ctx->use_f64 = !ctx->gold && (q < (1ull << 45)) && arith_mode() != 1;
        ctx->handoff_bytes = !ctx->coeff && handoff_is_packed(q, logn, ctx->use_f64) ? 6 : 8;
        const uint64_t w_last_scaled = ctx->coeff ? 0 : mulmod(tw.inv[n > 1 ? 1 : 0], tw.n_inv, q);
        if (ctx->coeff) {              // nothing to upload, and no transform ever reads the round constants
        } else if (ctx->gold) {   // multipliers in Montgomery form (gold_mul_mont)
            std::vector<uint64_t> f(n), g(n);
            for (uint32_t i = 0; i < n; ++i) {
                f[i] = prover_montgomery(tw.fwd[i]);
                g[i] = prover_montgomery(tw.inv[i]);
            }
            ctx->fwd_gold.upload(f);
            ctx->inv_gold.upload(g);
            ctx->n_inv_gold = prover_montgomery(tw.n_inv);
            ctx->w_last_scaled_gold = prover_montgomery(w_last_scaled);
        } else if (ctx->use_f64) {
            std::vector<double> f(n), g(n);
            for (uint32_t i = 0; i < n; ++i) {
                f[i] = static_cast<double>(tw.fwd[i]);
                g[i] = static_cast<double>(tw.inv[i]);
            }
            ctx->fwd_f64.upload(f);
            ctx->inv_f64.upload(g);
            ctx->n_inv_f64 = static_cast<double>(tw.n_inv);
            ctx->w_last_scaled_f64 = static_cast<double>(w_last_scaled);
        } else {
            std::vector<ShoupOperand> f(n), g(n);
            for (uint32_t i = 0; i < n; ++i) {
                f[i] = ShoupOperand{tw.fwd[i], shoup_quotient(tw.fwd[i], q)};
                g[i] = ShoupOperand{tw.inv[i], shoup_quotient(tw.inv[i], q)};
            }
            ctx->fwd_u64.upload(f);
            ctx->inv_u64.upload(g);
            ctx->n_inv_u64 = ShoupOperand{tw.n_inv, shoup_quotient(tw.n_inv, q)};
            ctx->w_last_scaled_u64 = ShoupOperand{w_last_scaled, shoup_quotient(w_last_scaled, q)};
        }
        ctx->staging.allocate(3ull * n);
    } catch (const std::exception& e) {
        set_last_error(std::string(where) + ": " + e.what());
        std::fprintf(stderr, "lambda_snark_core: %s failed: %s\n", where, e.what());
        return nullptr;
    }
    return ctx.release();
}

NttContext* create_ntt_context(uint64_t q, uint32_t n, int device) {
    int logn = 0;
    if (!ntt_params_valid(q, n, &logn)) {
        set_last_error("ntt_context_create: (q, n) rejected: need n = 2^k in [2,131072], prime q < 2^61, q = 1 mod 2n");
        return nullptr;
    }
    const uint64_t psi = minimal_primitive_root_2n(q, n);
    if (!psi) {
        set_last_error("ntt_context_create: no primitive 2n-th root");
        return nullptr;
    }
    return build_context("ntt_context_create", q, n, logn, device, build_twiddles(q, n, logn, psi), false);
}

NttContext* create_coeff_context(const char* where, uint64_t q, uint32_t n, int logn, int device) {
    return build_context(where, q, n, logn, device, TwiddleTables{}, false);
}

NttContext* create_cyclic_ntt_context(uint64_t q, uint32_t n, uint64_t omega, int device, bool large, const char* where) {
    if (omega == 0) omega = prover_root_of_unity(q, n);
    int logn = 0;
    if (!cyclic_params_valid(q, n, omega, &logn, large ? kProverMaxLog2 : kTwoPassMaxLog2)) {
        set_last_error(std::string(where) + ": need n = 2^k in [2," + std::to_string(1u << (large ? kProverMaxLog2 : kTwoPassMaxLog2)) +
                       "], prime q (NTT_MODULUS or < 2^61), omega of order n");
        return nullptr;
    }
    if (logn > kTwoPassMaxLog2 && q != kProverModulus) {   // the three-pass schedule exists in the Goldilocks flavour only (run_ntt)
        set_last_error(std::string(where) + ": n above 131072 needs q = NTT_MODULUS (the F64 / Shoup flavours stop at two passes)");
        return nullptr;
    }
    return build_context(where, q, n, logn, device, build_cyclic_twiddles(q, n, logn, omega), true);
}

hipStream_t work_stream(const NttContext& c) {
    std::lock_guard<std::mutex> lock(c.stream_mutex);
    if (!c.stream.handle) {
        DeviceGuard guard(c.device);
        LSR_HIP(hipStreamCreateWithFlags(&c.stream.handle, hipStreamNonBlocking));
    }
    return c.stream;
}

void destroy_ntt_context(NttContext* ctx) {
    if (!ctx) return;
    try {
        DeviceGuard guard(ctx->device);
        ctx->ring_event.sync();                     // a ring multiply still in flight may be using ring_scratch
        delete ctx;
    } catch (...) {
        delete ctx;
    }
}

// ------------------------------------------------------------------------------------------------
// dispatch
// ------------------------------------------------------------------------------------------------
template <class A, int LT, bool RAW_IN, bool RAW_OUT, bool PACKED = false>
static void tile_fwd(const NttContext& c, uint64_t* d, size_t total, hipStream_t s, const uint64_t* src = nullptr) {
    const unsigned grid = static_cast<unsigned>((total + kTile - 1) / kTile);
    hipLaunchKernelGGL((ntt_tile_forward<A, LT, RAW_IN, RAW_OUT, PACKED>), dim3(grid), dim3(kThreads), 0, s, d, total, c.mod, Flavour<A>::fwd(c), src);
}
template <class A, int LT, bool RAW_IN, bool RAW_OUT, bool DEFER = false, bool PACKED = false>
static void tile_inv(const NttContext& c, uint64_t* d, size_t total, hipStream_t s, const uint64_t* add = nullptr, const uint64_t* pre = nullptr) {
    const unsigned grid = static_cast<unsigned>((total + kTile - 1) / kTile);
    static_assert(!DEFER || !std::is_same_v<A, ArithGold>, "the pre-multiplied instantiation has no deferred form");
    if constexpr (std::is_same_v<A, ArithGold> && !RAW_IN) {   // the fused diagonal multiply exists for the prover's field only
        if (pre != nullptr) {
            hipLaunchKernelGGL((ntt_tile_inverse<A, LT, RAW_IN, RAW_OUT, true>), dim3(grid), dim3(kThreads), 0, s, d, total, c.mod, Flavour<A>::inv(c),
                               Flavour<A>::consts(c), add, pre);
            return;
        }
    }
    if (pre != nullptr) throw std::runtime_error("pre-multiplied inverse transform: only for NTT_MODULUS contexts");
    hipLaunchKernelGGL((ntt_tile_inverse<A, LT, RAW_IN, RAW_OUT, false, DEFER, PACKED>), dim3(grid), dim3(kThreads), 0, s, d, total, c.mod, Flavour<A>::inv(c),
                       Flavour<A>::consts(c), add);
}

// DEFERRED: the raw operands come from a tile pass that left its last round un-centred (run_ntt's two-pass inverse of a flavour with
// A::kDeferredRecentre): the round re-centres on load — the one class of words that can exceed 2 q for four stages, every word for five
// (lsr_ntt_kernels.hpp RECENTRE_IN, bounds in DESIGN.md §4; re-centring every word in the four-stage round measured the same,
// profiles/r12_inverse_tile_ablation.txt).  The pipelines that bring raw intermediates of their own (commitment, opening, ring
// multiply: launch_top_round_inverse, launch_strided_round) keep the plain instantiations.
// PACKED: the raw side is the 6-byte hand-off of run_ntt<ArithF64> (a two-pass transform's top round has four or five stages).
template <class A, bool INVERSE, bool RAW_IN, bool RAW_OUT, bool DEFERRED = false, bool PACKED = false>
static void strided(const NttContext& c, uint64_t* d, size_t total, int lo, int r, hipStream_t s, const uint64_t* add = nullptr) {
    constexpr int kOnLoad4 = DEFERRED ? 1 : 0, kOnLoad5 = DEFERRED ? 2 : 0;
    const size_t groups = total >> r;
    const unsigned grid = static_cast<unsigned>((groups + kThreads - 1) / kThreads);
    const auto* tw = INVERSE ? Flavour<A>::inv(c) : Flavour<A>::fwd(c);
    const auto cs = Flavour<A>::consts(c);
    if constexpr (PACKED) {
        static_assert(!DEFERRED, "the packed hand-off is re-centred by the tile pass");
        if (r != 4 && r != 5) throw std::runtime_error("packed hand-off: top rounds of four or five stages only");
        if constexpr (INVERSE) {
            if (add != nullptr) {
                if (r == 4) hipLaunchKernelGGL((ntt_strided_round<A, 4, true, true, false, true, 0, true>), dim3(grid), dim3(kThreads), 0, s, d, total, lo, c.mod, tw, cs, add);
                else hipLaunchKernelGGL((ntt_strided_round<A, 5, true, true, false, true, 0, true>), dim3(grid), dim3(kThreads), 0, s, d, total, lo, c.mod, tw, cs, add);
                return;
            }
        }
        if (r == 4) hipLaunchKernelGGL((ntt_strided_round<A, 4, INVERSE, RAW_IN, RAW_OUT, false, 0, true>), dim3(grid), dim3(kThreads), 0, s, d, total, lo, c.mod, tw, cs, add);
        else hipLaunchKernelGGL((ntt_strided_round<A, 5, INVERSE, RAW_IN, RAW_OUT, false, 0, true>), dim3(grid), dim3(kThreads), 0, s, d, total, lo, c.mod, tw, cs, add);
        return;
    }
    if constexpr (INVERSE && !RAW_OUT) {
        if (add != nullptr) {
            switch (r) {
                case 1: hipLaunchKernelGGL((ntt_strided_round<A, 1, true, RAW_IN, false, true, kOnLoad4>), dim3(grid), dim3(kThreads), 0, s, d, total, lo, c.mod, tw, cs, add); break;
                case 2: hipLaunchKernelGGL((ntt_strided_round<A, 2, true, RAW_IN, false, true, kOnLoad4>), dim3(grid), dim3(kThreads), 0, s, d, total, lo, c.mod, tw, cs, add); break;
                case 3: hipLaunchKernelGGL((ntt_strided_round<A, 3, true, RAW_IN, false, true, kOnLoad4>), dim3(grid), dim3(kThreads), 0, s, d, total, lo, c.mod, tw, cs, add); break;
                case 4: hipLaunchKernelGGL((ntt_strided_round<A, 4, true, RAW_IN, false, true, kOnLoad4>), dim3(grid), dim3(kThreads), 0, s, d, total, lo, c.mod, tw, cs, add); break;
                default: hipLaunchKernelGGL((ntt_strided_round<A, 5, true, RAW_IN, false, true, kOnLoad5>), dim3(grid), dim3(kThreads), 0, s, d, total, lo, c.mod, tw, cs, add); break;
            }
            return;
        }
    }
    switch (r) {
        case 1: hipLaunchKernelGGL((ntt_strided_round<A, 1, INVERSE, RAW_IN, RAW_OUT, false, kOnLoad4>), dim3(grid), dim3(kThreads), 0, s, d, total, lo, c.mod, tw, cs, add); break;
        case 2: hipLaunchKernelGGL((ntt_strided_round<A, 2, INVERSE, RAW_IN, RAW_OUT, false, kOnLoad4>), dim3(grid), dim3(kThreads), 0, s, d, total, lo, c.mod, tw, cs, add); break;
        case 3: hipLaunchKernelGGL((ntt_strided_round<A, 3, INVERSE, RAW_IN, RAW_OUT, false, kOnLoad4>), dim3(grid), dim3(kThreads), 0, s, d, total, lo, c.mod, tw, cs, add); break;
        case 4: hipLaunchKernelGGL((ntt_strided_round<A, 4, INVERSE, RAW_IN, RAW_OUT, false, kOnLoad4>), dim3(grid), dim3(kThreads), 0, s, d, total, lo, c.mod, tw, cs, add); break;
        default: hipLaunchKernelGGL((ntt_strided_round<A, 5, INVERSE, RAW_IN, RAW_OUT, false, kOnLoad5>), dim3(grid), dim3(kThreads), 0, s, d, total, lo, c.mod, tw, cs, add); break;
    }
}

// tile pass of a two-pass transform (n > 4096): LT low bits, raw element hand-off on the other side
template <class A, bool PACKED = false>
static void pass_forward(const NttContext& c, int lt, uint64_t* d, size_t total, hipStream_t s) {
    switch (lt) {
        case 9: tile_fwd<A, 9, true, false, PACKED>(c, d, total, s); break;
        case 10: tile_fwd<A, 10, true, false, PACKED>(c, d, total, s); break;
        case 11: tile_fwd<A, 11, true, false, PACKED>(c, d, total, s); break;
        default: tile_fwd<A, 12, true, false, PACKED>(c, d, total, s); break;
    }
}
template <class A, bool PACKED = false>
static void pass_inverse(const NttContext& c, int lt, uint64_t* d, size_t total, hipStream_t s, const uint64_t* pre) {
    // the strided round of run_ntt re-centres on load — unless the hand-off is packed: 6 bytes hold the re-centred words only
    constexpr bool kDefer = A::kDeferredRecentre && !PACKED;
    switch (lt) {
        case 9: tile_inv<A, 9, false, true, kDefer, PACKED>(c, d, total, s, nullptr, pre); break;
        case 10: tile_inv<A, 10, false, true, kDefer, PACKED>(c, d, total, s, nullptr, pre); break;
        case 11: tile_inv<A, 11, false, true, kDefer, PACKED>(c, d, total, s, nullptr, pre); break;
        default: tile_inv<A, 12, false, true, kDefer, PACKED>(c, d, total, s, nullptr, pre); break;
    }
}

template <class A>
static void small_forward(const NttContext& c, uint64_t* d, size_t total, hipStream_t s, const uint64_t* src) {
    switch (c.logn) {
        case 1: tile_fwd<A, 1, false, false>(c, d, total, s, src); break;
        case 2: tile_fwd<A, 2, false, false>(c, d, total, s, src); break;
        case 3: tile_fwd<A, 3, false, false>(c, d, total, s, src); break;
        case 4: tile_fwd<A, 4, false, false>(c, d, total, s, src); break;
        case 5: tile_fwd<A, 5, false, false>(c, d, total, s, src); break;
        case 6: tile_fwd<A, 6, false, false>(c, d, total, s, src); break;
        case 7: tile_fwd<A, 7, false, false>(c, d, total, s, src); break;
        case 8: tile_fwd<A, 8, false, false>(c, d, total, s, src); break;
        case 9: tile_fwd<A, 9, false, false>(c, d, total, s, src); break;
        case 10: tile_fwd<A, 10, false, false>(c, d, total, s, src); break;
        case 11: tile_fwd<A, 11, false, false>(c, d, total, s, src); break;
        default: tile_fwd<A, 12, false, false>(c, d, total, s, src); break;
    }
}
template <class A>
static void small_inverse(const NttContext& c, uint64_t* d, size_t total, hipStream_t s, const uint64_t* add, const uint64_t* pre) {
    switch (c.logn) {
        case 1: tile_inv<A, 1, false, false>(c, d, total, s, add, pre); break;
        case 2: tile_inv<A, 2, false, false>(c, d, total, s, add, pre); break;
        case 3: tile_inv<A, 3, false, false>(c, d, total, s, add, pre); break;
        case 4: tile_inv<A, 4, false, false>(c, d, total, s, add, pre); break;
        case 5: tile_inv<A, 5, false, false>(c, d, total, s, add, pre); break;
        case 6: tile_inv<A, 6, false, false>(c, d, total, s, add, pre); break;
        case 7: tile_inv<A, 7, false, false>(c, d, total, s, add, pre); break;
        case 8: tile_inv<A, 8, false, false>(c, d, total, s, add, pre); break;
        case 9: tile_inv<A, 9, false, false>(c, d, total, s, add, pre); break;
        case 10: tile_inv<A, 10, false, false>(c, d, total, s, add, pre); break;
        case 11: tile_inv<A, 11, false, false>(c, d, total, s, add, pre); break;
        default: tile_inv<A, 12, false, false>(c, d, total, s, add, pre); break;
    }
}

// Three-pass schedule of n = 2^18 .. 2^22: the top r_top index bits and the r_inner bits below them through one
// strided round each, the low lt bits through the tile kernel.  Radix-16 rounds wherever the size allows (5-stage rounds measured
// slower, profiles/README.md), the tile as large as possible.
struct LargeSchedule {
    int r_top, r_inner, lt;
};
static LargeSchedule large_schedule(int logn) {
    const int r_top = logn >= 21 ? 5 : 4, r_inner = logn >= 22 ? 5 : 4;
    return {r_top, r_inner, logn - r_top - r_inner};            // lt = 10, 11, 12, 12, 12
}
template <class A, bool INVERSE>
static void inner_round(const NttContext& c, uint64_t* d, size_t total, int lo, int r, hipStream_t s) {
    const unsigned grid = static_cast<unsigned>((total >> r) / kThreads);
    const auto* tw = INVERSE ? Flavour<A>::inv(c) : Flavour<A>::fwd(c);
    if (r == 4) hipLaunchKernelGGL((ntt_inner_round<A, 4, INVERSE>), dim3(grid), dim3(kThreads), 0, s, d, total, lo, c.mod, tw);
    else hipLaunchKernelGGL((ntt_inner_round<A, 5, INVERSE>), dim3(grid), dim3(kThreads), 0, s, d, total, lo, c.mod, tw);
}

size_t ntt_chunk_bytes() {
    static const size_t bytes = [] {
        if (const char* e = std::getenv("LAMBDA_SNARK_NTT_CHUNK_MIB")) {
            const long v = std::atol(e);
            if (v > 0) return static_cast<size_t>(v) << 20;
        }
        return static_cast<size_t>(256) << 20;
    }();
    return bytes;
}

template <class A>
static void run_ntt(const NttContext& c, uint64_t* d, size_t batch, bool inverse, hipStream_t s, const uint64_t* add, const uint64_t* pre,
                    const uint64_t* src) {
    const size_t total = batch << c.logn;
    if (total == 0) return;
    if (c.logn <= kTileLog) {
        if (inverse) small_inverse<A>(c, d, total, s, add, pre);
        else small_forward<A>(c, d, total, s, src);
        return;
    }
    // n > 4096: the top 4 (n = 2^17: 5) index bits go through ONE strided round, the low `lt` = 9..12 bits through the
    // tile kernel.  (5- and 6-stage strided rounds were measured slower at n = 2^16: profiles/README.md.)
    // n > 2^17: a second strided round between the two (large_schedule).
    const bool three = c.logn > kTwoPassMaxLog2;
    if (three && !std::is_same_v<A, ArithGold>) throw std::runtime_error("transforms above n = 131072: NTT_MODULUS contexts only");
    const LargeSchedule ls = three ? large_schedule(c.logn) : LargeSchedule{std::max(c.logn - kTileLog, 4), 0, 0};
    const int r_top = ls.r_top;
    const int lt = three ? ls.lt : c.logn - r_top;
    // Walk the batch in chunks small enough that the array written by one pass is still resident in the
    // 256 MiB Infinity Cache when the next pass reads it (MI355X_MICROARCH.md "Infinity Cache").
    const size_t chunk_polys = std::max<size_t>(1, ntt_chunk_bytes() >> (c.logn + 3));
    for (size_t first = 0; first < batch; first += chunk_polys) {
        const size_t now = std::min(chunk_polys, batch - first);
        uint64_t* base = d + (first << c.logn);
        const size_t count = now << c.logn;
        hipStream_t cs = s;
        if constexpr (std::is_same_v<A, ArithF64>) {
            if (c.handoff_bytes == 6) {   // the same two passes with the intermediate in 6 bytes per residue (build_context decided)
                if (!inverse) {
                    strided<A, false, false, true, false, true>(c, base, count, c.logn - r_top, r_top, cs, src ? src + (first << c.logn) : nullptr);
                    pass_forward<A, true>(c, lt, base, count, cs);
                } else {
                    pass_inverse<A, true>(c, lt, base, count, cs, pre);
                    strided<A, true, true, false, false, true>(c, base, count, c.logn - r_top, r_top, cs, add ? add + (first << c.logn) : nullptr);
                }
                continue;
            }
        }
        if (!inverse) {
            strided<A, false, false, true>(c, base, count, c.logn - r_top, r_top, cs, src ? src + (first << c.logn) : nullptr);
            if constexpr (std::is_same_v<A, ArithGold>) {
                if (three) inner_round<A, false>(c, base, count, lt, ls.r_inner, cs);
            }
            pass_forward<A>(c, lt, base, count, cs);
        } else {
            pass_inverse<A>(c, lt, base, count, cs, pre);
            if constexpr (std::is_same_v<A, ArithGold>) {
                if (three) inner_round<A, true>(c, base, count, lt, ls.r_inner, cs);
            }
            strided<A, true, true, false, A::kDeferredRecentre>(c, base, count, c.logn - r_top, r_top, cs, add ? add + (first << c.logn) : nullptr);
        }
    }
}

void launch_ntt(const NttContext& c, uint64_t* d, size_t batch, bool inverse, hipStream_t s, const uint64_t* add_on_inverse,
                const uint64_t* pre_mul_on_inverse, const uint64_t* forward_source) {
    const uint64_t* add = inverse ? add_on_inverse : nullptr;
    const uint64_t* pre = inverse ? pre_mul_on_inverse : nullptr;
    const uint64_t* src = inverse ? nullptr : forward_source;
    if (c.gold) run_ntt<ArithGold>(c, d, batch, inverse, s, add, pre, src);
    else if (c.use_f64) run_ntt<ArithF64>(c, d, batch, inverse, s, add, pre, src);
    else run_ntt<ArithU64>(c, d, batch, inverse, s, add, pre, src);
    LSR_HIP(hipGetLastError());
}

// Forward transform of a Goldilocks batch (n <= 4096: one tile launch) with elementwise work of the prover's quotient pipeline
// fused into its read-in (lsr_ntt_kernels.hpp, FuseIn): mode 1 = operands multiplied by x1 first, mode 2 = a b == c tested on the way in,
// mode 3 = mode 1 plus the quotient's finish on the way out (launch_ntt_forward_finish below).
template <int MODE>
static void fused_forward(const NttContext& c, uint64_t* d, size_t total, hipStream_t s, const uint64_t* src, const FuseIn& fuse) {
    const unsigned grid = static_cast<unsigned>((total + kTile - 1) / kTile);
    const auto* tw = Flavour<ArithGold>::fwd(c);
#define LSR_FUSED_CASE(LT) case LT: hipLaunchKernelGGL((ntt_tile_forward_fused<ArithGold, LT, MODE>), dim3(grid), dim3(kThreads), 0, s, d, total, c.mod, tw, src, fuse); break;
    switch (c.logn) {
        LSR_FUSED_CASE(1) LSR_FUSED_CASE(2) LSR_FUSED_CASE(3) LSR_FUSED_CASE(4) LSR_FUSED_CASE(5) LSR_FUSED_CASE(6)
        LSR_FUSED_CASE(7) LSR_FUSED_CASE(8) LSR_FUSED_CASE(9) LSR_FUSED_CASE(10) LSR_FUSED_CASE(11)
        default: hipLaunchKernelGGL((ntt_tile_forward_fused<ArithGold, 12, MODE>), dim3(grid), dim3(kThreads), 0, s, d, total, c.mod, tw, src, fuse); break;
    }
#undef LSR_FUSED_CASE
}
bool ntt_forward_can_fuse(const NttContext& c) { return c.gold && c.logn >= 1 && c.logn <= kTileLog; }
void launch_ntt_forward_fused(const NttContext& c, uint64_t* d, size_t batch, hipStream_t s, const uint64_t* src, int mode, const uint64_t* x1,
                              const uint64_t* x2, uint32_t* bad) {
    if (!ntt_forward_can_fuse(c) || (mode != 1 && mode != 2) || !x1 || (mode == 2 && (!x2 || !bad)))
        throw std::runtime_error("fused forward transform: Goldilocks context with n <= 4096, mode 1 or 2");
    const size_t total = batch << c.logn;
    if (!total) return;
    if (mode == 1) fused_forward<1>(c, d, total, s, src, FuseIn{x1, nullptr, nullptr});
    else fused_forward<2>(c, d, total, s, src, FuseIn{x1, x2, bad});
    LSR_HIP(hipGetLastError());
}

// Last transform of the quotient pipeline with both neighbours folded in: (d x1) on the way in, Q = (2m)^-1 c_hat - untwist z in natural
// order (and the per-instance degree bound `top`) on the way out; d is read only, z is never stored.
void launch_ntt_forward_finish(const NttContext& c, const uint64_t* d, size_t batch, hipStream_t s, const uint64_t* x1, const uint64_t* chat,
                               const uint64_t* untwist, uint64_t half_m_inv, uint64_t* quotient, uint32_t* top) {
    if (!ntt_forward_can_fuse(c) || !d || !x1 || !chat || !untwist || !quotient || !top)
        throw std::runtime_error("fused forward transform with finish: Goldilocks context with n <= 4096 and every operand");
    const size_t total = batch << c.logn;
    if (!total) return;
    FuseIn fuse{x1, nullptr, nullptr};
    fuse.chat = chat;
    fuse.untwist = untwist;
    fuse.half_m_inv = half_m_inv;
    fuse.quotient = quotient;
    fuse.top = top;
    fused_forward<3>(c, const_cast<uint64_t*>(d), total, s, nullptr, fuse);
    LSR_HIP(hipGetLastError());
}

// The strided (top index bits) round of an n > 4096 transform on its own: the outer passes of the fused commitment
// pipeline (lsr_commit.hip), whose middle stage replaces the tile kernels.  FP64 flavour.
void launch_top_round_forward(const NttContext& c, uint64_t* dst, const uint64_t* src, size_t polys, hipStream_t s) {
    if (!c.use_f64 || c.logn <= kTileLog) throw std::runtime_error("top-round launch: FP64 flavour, n > 4096 only");
    const int r_top = std::max(c.logn - kTileLog, 4);
    strided<ArithF64, false, false, true>(c, dst, polys << c.logn, c.logn - r_top, r_top, s, src);
    LSR_HIP(hipGetLastError());
}
void launch_top_round_inverse(const NttContext& c, uint64_t* data, size_t polys, hipStream_t s, const uint64_t* add) {
    if (!c.use_f64 || c.logn <= kTileLog) throw std::runtime_error("top-round launch: FP64 flavour, n > 4096 only");
    const int r_top = std::max(c.logn - kTileLog, 4);
    strided<ArithF64, true, true, false>(c, data, polys << c.logn, c.logn - r_top, r_top, s, add);
    LSR_HIP(hipGetLastError());
}

// The strided round of an n > 4096 transform in any flavour (the outer passes of the ring multiply, lsr_ring_mul.hip): forward reads
// canonical `src` and writes raw elements to `d` (may alias); inverse turns raw elements of `d` into canonical residues in place.
void launch_strided_round(const NttContext& c, uint64_t* d, const uint64_t* src, size_t polys, bool inverse, hipStream_t s) {
    if (c.logn <= kTileLog || c.logn > kTwoPassMaxLog2) throw std::runtime_error("strided round: 4096 < n <= 131072 only");
    const int r_top = std::max(c.logn - kTileLog, 4), lo = c.logn - r_top;
    const size_t total = polys << c.logn;
    if (inverse) {
        if (c.gold) strided<ArithGold, true, true, false>(c, d, total, lo, r_top, s);
        else if (c.use_f64) strided<ArithF64, true, true, false>(c, d, total, lo, r_top, s);
        else strided<ArithU64, true, true, false>(c, d, total, lo, r_top, s);
    } else {
        if (c.gold) strided<ArithGold, false, false, true>(c, d, total, lo, r_top, s, src);
        else if (c.use_f64) strided<ArithF64, false, false, true>(c, d, total, lo, r_top, s, src);
        else strided<ArithU64, false, false, true>(c, d, total, lo, r_top, s, src);
    }
    LSR_HIP(hipGetLastError());
}

void launch_top_round_inverse_sampled(const NttContext& c, uint64_t* data, size_t polys, hipStream_t s, const BlindSampler& bs) {
    if (!c.use_f64 || c.logn <= kTileLog) throw std::runtime_error("top-round launch: FP64 flavour, n > 4096 only");
    const int r_top = std::max(c.logn - kTileLog, 4), lo = c.logn - r_top;
    const size_t total = polys << c.logn;
    const unsigned grid = static_cast<unsigned>(((total >> r_top) + kThreads - 1) / kThreads);
    const bool half = bs.side != nullptr;                                 // rows [0, 2^r / 2) were sampled by the forward round
    const unsigned lds = (((bs.entries + 1u) & ~1u) * 8u) + ((kThreads << r_top) >> (half ? 1 : 0)) * 4u;   // table + int32 tile
    const auto cs = Flavour<ArithF64>::consts(c);
    const auto* tw = Flavour<ArithF64>::inv(c);
    if (r_top == 4 && !half) hipLaunchKernelGGL((ntt_strided_round_sampled<ArithF64, 4, true, false>), dim3(grid), dim3(kThreads), lds, s, data, total, lo, c.mod, tw, cs, bs);
    else if (r_top == 4) hipLaunchKernelGGL((ntt_strided_round_sampled<ArithF64, 4, true, true>), dim3(grid), dim3(kThreads), lds, s, data, total, lo, c.mod, tw, cs, bs);
    else if (r_top == 5 && !half) hipLaunchKernelGGL((ntt_strided_round_sampled<ArithF64, 5, true, false>), dim3(grid), dim3(kThreads), lds, s, data, total, lo, c.mod, tw, cs, bs);
    else if (r_top == 5) hipLaunchKernelGGL((ntt_strided_round_sampled<ArithF64, 5, true, true>), dim3(grid), dim3(kThreads), lds, s, data, total, lo, c.mod, tw, cs, bs);
    else throw std::runtime_error("top-round launch: 4 or 5 top bits only");
    LSR_HIP(hipGetLastError());
}

void launch_top_round_forward_sampling(const NttContext& c, uint64_t* dst, const uint64_t* src, size_t polys, hipStream_t s, const BlindSampler& bs) {
    if (!c.use_f64 || c.logn <= kTileLog) throw std::runtime_error("top-round launch: FP64 flavour, n > 4096 only");
    if (!bs.side || bs.entries > 127) throw std::runtime_error("forward sampling: side buffer and a table of <= 127 entries needed");
    const int r_top = std::max(c.logn - kTileLog, 4), lo = c.logn - r_top;
    const size_t total = polys << c.logn;
    const unsigned grid = static_cast<unsigned>(((total >> r_top) + kThreads - 1) / kThreads);
    const unsigned lds = (((bs.entries + 1u) & ~1u) * 8u) + ((kThreads << r_top) >> 1);                      // table + int8 tile
    const auto cs = Flavour<ArithF64>::consts(c);
    const auto* tw = Flavour<ArithF64>::fwd(c);
    if (r_top == 4) hipLaunchKernelGGL((ntt_strided_round_sampling<ArithF64, 4>), dim3(grid), dim3(kThreads), lds, s, dst, total, lo, c.mod, tw, cs, src, bs);
    else if (r_top == 5) hipLaunchKernelGGL((ntt_strided_round_sampling<ArithF64, 5>), dim3(grid), dim3(kThreads), lds, s, dst, total, lo, c.mod, tw, cs, src, bs);
    else throw std::runtime_error("top-round launch: 4 or 5 top bits only");
    LSR_HIP(hipGetLastError());
}

void launch_pointwise(const NttContext& c, uint64_t* out, const uint64_t* a, const uint64_t* b, size_t count, hipStream_t s) {
    if (!count) return;
    const size_t want = (count + kThreads - 1) / kThreads;
    const unsigned grid = static_cast<unsigned>(std::min<size_t>(want, 256 * 16));
    if (c.gold) hipLaunchKernelGGL(pointwise_mul_gold_kernel, dim3(grid), dim3(kThreads), 0, s, out, a, b, count);
    else hipLaunchKernelGGL(pointwise_mul_kernel, dim3(grid), dim3(kThreads), 0, s, out, a, b, count, c.mod);
    LSR_HIP(hipGetLastError());
}

void launch_bit_reverse(uint64_t* out, const uint64_t* in, int logn, size_t batch, hipStream_t s) {
    const size_t total = batch << logn;
    if (!total) return;
    const unsigned grid = static_cast<unsigned>(std::min<size_t>((total + kThreads - 1) / kThreads, 256 * 32));
    hipLaunchKernelGGL(bit_reverse_kernel, dim3(grid), dim3(kThreads), 0, s, out, in, logn, total);
    LSR_HIP(hipGetLastError());
}

// host-buffer transform of `batch` polynomials through bounded device chunks
static void host_ntt(const NttContext& c, uint64_t* polys, size_t batch, bool inverse) {
    DeviceGuard guard(c.device);
    const size_t n = c.degree;
    if (batch == 1) {
        std::lock_guard<std::mutex> lock(c.staging_mutex);
        LSR_HIP(hipMemcpyAsync(c.staging.ptr, polys, n * 8, hipMemcpyHostToDevice, work_stream(c)));
        launch_ntt(c, c.staging.ptr, 1, inverse, work_stream(c));
        LSR_HIP(hipMemcpyAsync(polys, c.staging.ptr, n * 8, hipMemcpyDeviceToHost, work_stream(c)));
        LSR_HIP(hipStreamSynchronize(work_stream(c)));
        return;
    }
    const size_t chunk_polys = std::max<size_t>(1, std::min<size_t>(batch, (512ull << 20) / (n * 8)));
    DeviceBuffer<uint64_t> buf(chunk_polys * n);
    std::lock_guard<std::mutex> lock(c.staging_mutex);   // serialises use of work_stream(c)
    for (size_t done = 0; done < batch; done += chunk_polys) {
        const size_t now = std::min(chunk_polys, batch - done);
        LSR_HIP(hipMemcpyAsync(buf.ptr, polys + done * n, now * n * 8, hipMemcpyHostToDevice, work_stream(c)));
        launch_ntt(c, buf.ptr, now, inverse, work_stream(c));
        LSR_HIP(hipMemcpyAsync(polys + done * n, buf.ptr, now * n * 8, hipMemcpyDeviceToHost, work_stream(c)));
        LSR_HIP(hipStreamSynchronize(work_stream(c)));
    }
}

static void host_pointwise(const NttContext& c, uint64_t* result, const uint64_t* a, const uint64_t* b, size_t count) {
    if (!count) return;
    DeviceGuard guard(c.device);
    std::lock_guard<std::mutex> lock(c.staging_mutex);
    DeviceBuffer<uint64_t> big;
    uint64_t* base = c.staging.ptr;
    if (3 * count > c.staging.count) {
        big.allocate(3 * count);
        base = big.ptr;
    }
    uint64_t* da = base;
    uint64_t* db = base + count;
    uint64_t* dr = base + 2 * count;
    LSR_HIP(hipMemcpyAsync(da, a, count * 8, hipMemcpyHostToDevice, work_stream(c)));
    LSR_HIP(hipMemcpyAsync(db, b, count * 8, hipMemcpyHostToDevice, work_stream(c)));
    launch_pointwise(c, dr, da, db, count, work_stream(c));
    LSR_HIP(hipMemcpyAsync(result, dr, count * 8, hipMemcpyDeviceToHost, work_stream(c)));
    LSR_HIP(hipStreamSynchronize(work_stream(c)));
}

}  // namespace lsr

// ------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------
using lsr::abi_guarded;
using lsr::set_last_error;

extern "C" {

int lsr_device_count(void) noexcept { return lsr::visible_device_count(); }
const char* lsr_last_error(void) noexcept { return lsr::last_error_cstr(); }
const char* lsr_version(void) noexcept { return "lambda_snark_core hip gfx950 r3 (f64-FMA Barrett + u64 Shoup NTT; fused tile pipeline for commitments and openings)"; }
void lsr_set_arith_mode(int mode) noexcept { lsr::g_arith_mode.store(mode); }

NttContext* ntt_context_create(uint64_t q, uint32_t n) noexcept {
    try {
        return lsr::create_ntt_context(q, n, -1);
    } catch (...) {
        return nullptr;
    }
}
NttContext* lsr_ntt_context_create_on(uint64_t q, uint32_t n, int device) noexcept {
    try {
        return lsr::create_ntt_context(q, n, device);
    } catch (...) {
        return nullptr;
    }
}
void ntt_context_free(NttContext* ctx) noexcept {
    if (ctx && ctx->coeff) return;   // lent by a ring handle and freed with it
    lsr::destroy_ntt_context(ctx);
}
int lsr_ntt_context_device(const NttContext* ctx) noexcept { return ctx ? ctx->device : -1; }
uint64_t lsr_ntt_context_root(const NttContext* ctx) noexcept { return ctx ? ctx->psi : 0; }
int lsr_ntt_context_uses_f64(const NttContext* ctx) noexcept { return ctx && ctx->use_f64 ? 1 : 0; }
int lsr_ntt_handoff_bytes(const NttContext* ctx) noexcept { return ctx ? ctx->handoff_bytes : -1; }

int ntt_forward(const NttContext* ctx, uint64_t* coeffs, uint32_t n) noexcept {
    if (lsr::refuse_coeff_context("ntt_forward", ctx)) return -1;
    if (!ctx || !coeffs || n != ctx->degree) return -1;   // ntt.cpp:81
    return abi_guarded("ntt_forward", [&] { lsr::host_ntt(*ctx, coeffs, 1, false); });
}
int ntt_inverse(const NttContext* ctx, uint64_t* evals, uint32_t n) noexcept {
    if (lsr::refuse_coeff_context("ntt_inverse", ctx)) return -1;
    if (!ctx || !evals || n != ctx->degree) return -1;    // ntt.cpp:96
    return abi_guarded("ntt_inverse", [&] { lsr::host_ntt(*ctx, evals, 1, true); });
}
void ntt_mul_pointwise(const NttContext* ctx, uint64_t* result, const uint64_t* a, const uint64_t* b, uint32_t n) noexcept {
    if (!ctx || !result || !a || !b) return;              // ntt.cpp:113
    (void)abi_guarded("ntt_mul_pointwise", [&] { lsr::host_pointwise(*ctx, result, a, b, n); });
}

int ntt_forward_batch(const NttContext* ctx, uint64_t* polys, size_t batch) noexcept {
    if (lsr::refuse_coeff_context("ntt_forward_batch", ctx)) return -1;
    if (!ctx || !polys) return -1;
    if (batch == 0) return 0;
    return abi_guarded("ntt_forward_batch", [&] { lsr::host_ntt(*ctx, polys, batch, false); });
}
int ntt_inverse_batch(const NttContext* ctx, uint64_t* polys, size_t batch) noexcept {
    if (lsr::refuse_coeff_context("ntt_inverse_batch", ctx)) return -1;
    if (!ctx || !polys) return -1;
    if (batch == 0) return 0;
    return abi_guarded("ntt_inverse_batch", [&] { lsr::host_ntt(*ctx, polys, batch, true); });
}
int ntt_mul_pointwise_batch(const NttContext* ctx, uint64_t* result, const uint64_t* a, const uint64_t* b, size_t batch) noexcept {
    if (!ctx || !result || !a || !b) return -1;
    return abi_guarded("ntt_mul_pointwise_batch", [&] { lsr::host_pointwise(*ctx, result, a, b, batch * ctx->degree); });
}

int lsr_ntt_forward_batch_device(const NttContext* ctx, uint64_t* d_polys, size_t batch, void* stream) noexcept {
    if (lsr::refuse_coeff_context("lsr_ntt_forward_batch_device", ctx)) return -1;
    if (!ctx || !d_polys) return -1;
    return abi_guarded("lsr_ntt_forward_batch_device", [&] {
        lsr::DeviceGuard guard(ctx->device);
        lsr::launch_ntt(*ctx, d_polys, batch, false, static_cast<hipStream_t>(stream));
    });
}
int lsr_ntt_inverse_batch_device(const NttContext* ctx, uint64_t* d_polys, size_t batch, void* stream) noexcept {
    if (lsr::refuse_coeff_context("lsr_ntt_inverse_batch_device", ctx)) return -1;
    if (!ctx || !d_polys) return -1;
    return abi_guarded("lsr_ntt_inverse_batch_device", [&] {
        lsr::DeviceGuard guard(ctx->device);
        lsr::launch_ntt(*ctx, d_polys, batch, true, static_cast<hipStream_t>(stream));
    });
}
int lsr_ntt_mul_pointwise_device(const NttContext* ctx, uint64_t* d_result, const uint64_t* d_a, const uint64_t* d_b, size_t count,
                                 void* stream) noexcept {
    if (!ctx || !d_result || !d_a || !d_b) return -1;
    return abi_guarded("lsr_ntt_mul_pointwise_device", [&] {
        lsr::DeviceGuard guard(ctx->device);
        lsr::launch_pointwise(*ctx, d_result, d_a, d_b, count, static_cast<hipStream_t>(stream));
    });
}

/* ---- multi-device sharding: contiguous slices, one host thread per shard, no collective ---- */
void lsr_shard_bounds(size_t batch, int shards, int index, size_t* first, size_t* count) noexcept {
    size_t lo = 0, len = 0;
    if (shards > 0 && index >= 0 && index < shards) {
        const size_t base = batch / (size_t)shards, extra = batch % (size_t)shards;
        lo = (size_t)index * base + std::min<size_t>((size_t)index, extra);
        len = base + ((size_t)index < extra ? 1 : 0);
    }
    if (first) *first = lo;
    if (count) *count = len;
}

void* lsr_host_alloc_pinned(size_t bytes) noexcept {
    void* p = nullptr;
    if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocPortable)   /* every device of the node may DMA into it */ != hipSuccess) return nullptr;
    return p;
}
void lsr_host_free_pinned(void* p) noexcept {
    if (p) (void)hipHostFree(p);
}

static int ntt_batch_sharded(const char* where, const NttContext* const* ctxs, int shards, uint64_t* polys, size_t batch, bool inverse) noexcept {
    if (!ctxs || shards <= 0) return -1;
    for (int g = 0; g < shards; ++g)
        if (lsr::refuse_coeff_context(where, ctxs[g])) return -1;
    if (!polys) return -1;
    for (int g = 0; g < shards; ++g)
        if (!ctxs[g] || ctxs[g]->degree != ctxs[0]->degree || ctxs[g]->modulus != ctxs[0]->modulus) return -1;
    if (batch == 0) return 0;
    std::vector<int> rc(shards, 0);
    std::vector<std::string> errors(shards);
    std::vector<std::thread> pool;
    for (int g = 0; g < shards; ++g)
        pool.emplace_back([&, g] {
            size_t first = 0, count = 0;
            lsr_shard_bounds(batch, shards, g, &first, &count);
            if (count == 0) return;
            try {
                lsr::host_ntt(*ctxs[g], polys + first * ctxs[g]->degree, count, inverse);   // H2D, transform, D2H straight into the caller's array
            } catch (const std::exception& e) {
                rc[g] = -1;
                errors[g] = e.what();
            } catch (...) {
                rc[g] = -1;
            }
        });
    for (std::thread& th : pool) th.join();
    for (int g = 0; g < shards; ++g)
        if (rc[g] != 0) {
            set_last_error(std::string(where) + ": shard " + std::to_string(g) + ": " + errors[g]);
            std::fprintf(stderr, "lambda_snark_core: %s failed on shard %d: %s\n", where, g, errors[g].c_str());
            return -1;
        }
    return 0;
}
int lsr_ntt_forward_batch_sharded(const NttContext* const* ctxs, int shards, uint64_t* polys, size_t batch) noexcept {
    return ntt_batch_sharded("lsr_ntt_forward_batch_sharded", ctxs, shards, polys, batch, false);
}
int lsr_ntt_inverse_batch_sharded(const NttContext* const* ctxs, int shards, uint64_t* polys, size_t batch) noexcept {
    return ntt_batch_sharded("lsr_ntt_inverse_batch_sharded", ctxs, shards, polys, batch, true);
}

uint64_t lsr_minimal_primitive_root(uint64_t q, uint32_t n) noexcept {
    int logn = 0;
    if (!lsr::ntt_params_valid(q, n, &logn)) return 0;
    return lsr::minimal_primitive_root_2n(q, n);
}
uint64_t lsr_select_commit_modulus(uint64_t requested_q, uint32_t n) noexcept { return lsr::select_commit_modulus(requested_q, n); }
uint64_t lsr_plain_modulus(uint32_t n) noexcept { return lsr::plain_modulus_for(n); }
size_t lsr_gaussian_cdf(double sigma, uint64_t* cdf, size_t cap) noexcept {
    try {
        const std::vector<uint64_t> table = lsr::gaussian_cdf(sigma);
        if (table.empty() || table.size() > cap || !cdf) return 0;
        std::memcpy(cdf, table.data(), table.size() * sizeof(uint64_t));
        return table.size();
    } catch (...) {
        return 0;
    }
}

}  // extern "C"
