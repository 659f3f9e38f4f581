// Operator-norm-bounded ring challenges (batch.h "operator-norm-bounded ring challenges"): the fixed-point operator
// norm N(c) of ring elements, and challenges with kappa1 coefficients +-1 and kappa2 coefficients +-2 drawn from the ChaCha20
// streams of lsr_ring_sample.hip and resampled on the device until N(c) <= T^2 2^60.  Integer code that reads only q, n and the
// ring of the context: one path for every flavour and both rings, n <= 4096.  The cosine table is built on the host and cached
// in the context; behind lsr_ntt_ring_opnorm_prepare the device forms enqueue one kernel and nothing else.
#include <algorithm>
#include <cmath>
#include <vector>

#include "lambda_snark/batch.h"
#include "lsr_ring_call.hpp"
#include "lsr_ring_challenge_kernels.hpp"
#include "lsr_runtime.hpp"

namespace lsr {

static_assert(kChallengeAttemptWords == LSR_RING_CHALLENGE_ATTEMPT_WORDS && kChallengeMaxTries == LSR_RING_CHALLENGE_MAX_TRIES,
              "batch.h and the kernels agree on the stream layout of the attempts");
static_assert(1u << kOpnormMaxLog == LSR_RING_OPNORM_MAX_DEGREE, "batch.h and the kernels agree on the largest ring degree");
// an attempt's word indices a kappa + s (a < 64, s < kappa <= n <= 4096) stay inside its 2^18 words, and all attempts below 2^28:
// the 32-bit block counter never wraps
static_assert((uint64_t)LSR_RING_SAMPLE_MAX_WORDS * LSR_RING_OPNORM_MAX_DEGREE <= LSR_RING_CHALLENGE_ATTEMPT_WORDS, "64 n <= 2^18");
static_assert((uint64_t)LSR_RING_CHALLENGE_MAX_TRIES * LSR_RING_CHALLENGE_ATTEMPT_WORDS <= 1ull << 28, "max_tries 2^18 <= 2^28");
static_assert(LSR_RING_CHALLENGE_ATTEMPT_WORDS % 8 == 0, "an attempt starts on a stream block");
// the largest workgroup (n = 4096, kappa = n, one wave) fits the LDS bound
static_assert(8u * 4096 + kChallengeChunkWords * 8 + 4096 / 2 + 4096 * 2 <= kChallengeLdsBytes, "table + words + codes + pairs");

static bool power_of_two_in_range(uint64_t n) { return n >= 2 && n <= LSR_RING_OPNORM_MAX_DEGREE && (n & (n - 1)) == 0; }

// C[j] = round(2^30 cos(pi j / n)), 0 <= j < 2n (no entry is near a rounding tie: DESIGN.md §5n)
static void opnorm_table(uint32_t n, int32_t* out) {
    for (uint32_t j = 0; j < 2 * n; ++j) out[j] = (int32_t)std::llround(std::ldexp(std::cos(M_PI * (double)j / (double)n), 30));
}

// the context's table on its device (caller holds a DeviceGuard); the first call builds and uploads it, synchronously
static const int32_t* resident_table(const NttContext& c, hipStream_t s) {
    std::lock_guard<std::mutex> lock(c.opnorm_mutex);
    if (!c.opnorm_table.ptr) {
        if (stream_is_capturing(s))
            throw std::runtime_error("the operator-norm table of this context is not resident yet and a capturing stream cannot upload it: call "
                                     "lsr_ntt_ring_opnorm_prepare (or make one eager call) before capturing");
        std::vector<int32_t> host(2 * (size_t)c.degree);
        opnorm_table(c.degree, host.data());
        c.opnorm_table.upload(host);
    }
    return c.opnorm_table.ptr;
}

static std::string degree_refusal(const NttContext& c) {
    return "n = " + std::to_string(c.degree) + " is above LSR_RING_OPNORM_MAX_DEGREE = " + std::to_string(LSR_RING_OPNORM_MAX_DEGREE) +
           ", the largest ring degree of the operator norm";
}

static void opnorm_device(const NttContext& c, const uint64_t* d_x, size_t count, uint64_t* d_out, const int32_t* d_table, hipStream_t s) {
    const OpnormJob job{d_out, d_x, d_table, count, c.modulus, (uint32_t)c.logn, c.cyclic ? 1u : 0u};
    const unsigned threads = c.degree <= 128 ? 64 : 256;      // n / 2 (+ 1) points: one wave holds them all at n <= 128
    const unsigned grid = static_cast<unsigned>(std::min<size_t>(count, 1u << 20));
    hipLaunchKernelGGL(ring_opnorm_kernel, dim3(grid), dim3(threads), (size_t)c.degree * 12, s, job);
    LSR_HIP(hipGetLastError());
}

struct ChallengeCall {
    uint32_t kappa1, kappa2, max_tries;
    uint64_t bound;           // T, below 2^32; 0: no check
    uint64_t components;      // min(components, count)
    uint32_t domain;
    uint64_t index_base;
};

// elements [first, first + count) of a call (element `first` at d_out and d_tries); d_keys holds the key groups from group_base on
static void challenge_device(const NttContext& c, uint64_t* d_out, int32_t* d_tries, uint64_t first, uint64_t count, const ChallengeCall& call,
                             const uint64_t* d_keys, uint64_t group_base, const int32_t* d_table, hipStream_t s) {
    ChallengeJob job{};
    job.out = d_out;
    job.tries = d_tries;
    job.keys = d_keys;
    job.table = d_table;
    job.index_base = call.index_base;
    job.components = call.components;
    job.group_base = group_base;
    job.first = first;
    job.count = count;
    job.q = c.modulus;
    const uint64_t t2 = call.bound * call.bound;              // T < 2^32
    job.bound_lo = t2 << 60;
    job.bound_hi = t2 >> 4;
    job.kappa1 = call.kappa1;
    job.kappa2 = call.kappa2;
    job.max_tries = call.max_tries;
    job.check = call.bound != 0;
    job.domain = call.domain;
    job.logn = (uint32_t)c.logn;
    job.cyclic = c.cyclic ? 1u : 0u;
    const ChallengeLayout lay = challenge_layout(c.degree, call.kappa1 + call.kappa2, job.check != 0);
    const uint64_t fit = (kChallengeLdsBytes - lay.table_bytes) / lay.wave_bytes;      // at least 1 (static_assert above)
    job.waves = (uint32_t)std::min<uint64_t>({(uint64_t)kChallengeMaxWaves, fit, count});
    const size_t bytes = lay.table_bytes + (size_t)job.waves * lay.wave_bytes;
    const unsigned grid = static_cast<unsigned>(std::min<uint64_t>((count + job.waves - 1) / job.waves, 1u << 20));
    hipLaunchKernelGGL(ring_challenge_kernel, dim3(grid), dim3(64 * job.waves), bytes, s, job);
    LSR_HIP(hipGetLastError());
}

}  // namespace lsr

// ------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------
namespace {

int opnorm_call(const char* where, const NttContext* ctx, const uint64_t* x, size_t count, uint64_t* out, bool device, void* stream) noexcept {
    if (!ctx || !x || !out) return lsr::abi_refuse(where, "NULL context or buffer");
    if (ctx->degree > LSR_RING_OPNORM_MAX_DEGREE) return lsr::abi_refuse(where, lsr::degree_refusal(*ctx));
    if (count == 0) return 0;
    return lsr::abi_guarded(where, [&] {
        size_t bytes = 0;
        if (__builtin_mul_overflow(count, (size_t)ctx->degree * 8, &bytes)) throw std::runtime_error("the sizes of the buffers overflow size_t");
        lsr::require_apart(out, count * 16, x, bytes, "out overlaps x: the output must not share memory with the operand");
        lsr::require_device();
        lsr::DeviceGuard guard(ctx->device);
        if (device) {
            hipStream_t s = static_cast<hipStream_t>(stream);
            lsr::opnorm_device(*ctx, x, count, out, lsr::resident_table(*ctx, s), s);
        } else {
            const int32_t* d_table = lsr::resident_table(*ctx, nullptr);
            lsr::host_staged(*ctx, out, x, count, 2, ctx->degree, [&](uint64_t* d_out, const uint64_t* d_in, size_t now, hipStream_t s) {
                lsr::opnorm_device(*ctx, d_in, now, d_out, d_table, s);
            });
        }
    });
}

int challenge_call(const char* where, const NttContext* ctx, uint64_t* out, int32_t* tries, size_t count, uint32_t kappa1, uint32_t kappa2,
                   uint64_t opnorm_bound, uint32_t max_tries, const uint64_t* keys, size_t components, uint32_t domain, uint64_t index_base,
                   bool device, void* stream) noexcept {
    // (1), (2) read nothing; (3), (4) read n and q of the context; (5), (6) read nothing; (7) reads n
    if (!ctx || !out || !tries || !keys) return lsr::abi_refuse(where, "NULL context, buffer, tries or keys");
    if (components == 0) return lsr::abi_refuse(where, "components must be at least 1");
    const uint64_t kappa = (uint64_t)kappa1 + kappa2;
    if (kappa == 0 || kappa > ctx->degree)
        return lsr::abi_refuse(where, "kappa1 + kappa2 = " + std::to_string(kappa) + " is not in 1 .. n = " + std::to_string(ctx->degree));
    if (kappa2 > 0 && ctx->modulus < 5)
        return lsr::abi_refuse(where, "kappa2 > 0 takes a modulus of at least 5 (2 and q - 2 next to 1 and q - 1), not q = " + std::to_string(ctx->modulus));
    if (max_tries == 0 || max_tries > LSR_RING_CHALLENGE_MAX_TRIES)
        return lsr::abi_refuse(where, "max_tries = " + std::to_string(max_tries) + " is not in 1 .. LSR_RING_CHALLENGE_MAX_TRIES = " +
                                          std::to_string(LSR_RING_CHALLENGE_MAX_TRIES));
    if (opnorm_bound >> 32) return lsr::abi_refuse(where, "opnorm_bound = " + std::to_string(opnorm_bound) + " is not below 2^32");
    if (ctx->degree > LSR_RING_OPNORM_MAX_DEGREE) return lsr::abi_refuse(where, lsr::degree_refusal(*ctx));
    if (count == 0) return 0;
    return lsr::abi_guarded(where, [&] {
        if (index_base + components < index_base) throw std::runtime_error("index_base + components overflows 64 bits");
        lsr::require_device();
        const lsr::ChallengeCall call{kappa1, kappa2, max_tries, opnorm_bound, std::min<uint64_t>(components, count), domain, index_base};
        lsr::DeviceGuard guard(ctx->device);
        if (device) {
            hipStream_t s = static_cast<hipStream_t>(stream);
            const int32_t* d_table = opnorm_bound ? lsr::resident_table(*ctx, s) : nullptr;
            lsr::challenge_device(*ctx, out, tries, 0, count, call, keys, 0, d_table, s);
        } else {
            const int32_t* d_table = opnorm_bound ? lsr::resident_table(*ctx, nullptr) : nullptr;
            // host buffers through bounded device chunks of whole elements; each chunk brings its own key groups and takes its tries back
            const size_t n = ctx->degree;
            lsr::host_staged(*ctx, count, lsr::staging_chunk(count, n + 1),
                             {lsr::staged_groups(keys, 32, call.components), lsr::staged_items(nullptr, out, n * 8), lsr::staged_items(nullptr, tries, 4)},
                             [&](const lsr::StagedChunk& k, hipStream_t s) {
                                 lsr::challenge_device(*ctx, k.lane<uint64_t>(1), k.lane<int32_t>(2), k.first, k.now, call, k.lane<const uint64_t>(0), k.group_first, d_table, s);
                             });
        }
    });
}

}  // namespace

extern "C" {

int lsr_ring_opnorm_table(uint32_t n, int32_t* out) noexcept {
    if (!out) return lsr::abi_refuse("lsr_ring_opnorm_table", "NULL buffer");
    if (!lsr::power_of_two_in_range(n))
        return lsr::abi_refuse("lsr_ring_opnorm_table", "n = " + std::to_string(n) + " is not a power of two in 2 .. LSR_RING_OPNORM_MAX_DEGREE = " +
                                                            std::to_string(LSR_RING_OPNORM_MAX_DEGREE));
    lsr::opnorm_table(n, out);
    return 0;
}

int lsr_ntt_ring_opnorm_prepare(const NttContext* ctx) noexcept {
    const char* const where = "lsr_ntt_ring_opnorm_prepare";
    if (!ctx) return lsr::abi_refuse(where, "NULL context");
    if (ctx->degree > LSR_RING_OPNORM_MAX_DEGREE) return lsr::abi_refuse(where, lsr::degree_refusal(*ctx));
    return lsr::abi_guarded(where, [&] {
        lsr::require_device();
        lsr::DeviceGuard guard(ctx->device);
        lsr::resident_table(*ctx, nullptr);
    });
}

int lsr_ntt_ring_opnorm_batch(const NttContext* ctx, const uint64_t* x, size_t count, uint64_t* out) noexcept {
    return opnorm_call("lsr_ntt_ring_opnorm_batch", ctx, x, count, out, false, nullptr);
}
int lsr_ntt_ring_opnorm_batch_device(const NttContext* ctx, const uint64_t* d_x, size_t count, uint64_t* d_out, void* stream) noexcept {
    return opnorm_call("lsr_ntt_ring_opnorm_batch_device", ctx, d_x, count, d_out, true, stream);
}

int lsr_ntt_ring_challenge_batch(const NttContext* ctx, uint64_t* out, int32_t* tries, size_t count, uint32_t kappa1, uint32_t kappa2,
                                 uint64_t opnorm_bound, uint32_t max_tries, const uint64_t* keys, size_t components, uint32_t domain,
                                 uint64_t index_base) noexcept {
    return challenge_call("lsr_ntt_ring_challenge_batch", ctx, out, tries, count, kappa1, kappa2, opnorm_bound, max_tries, keys, components, domain,
                          index_base, false, nullptr);
}
int lsr_ntt_ring_challenge_batch_device(const NttContext* ctx, uint64_t* d_out, int32_t* d_tries, size_t count, uint32_t kappa1, uint32_t kappa2,
                                        uint64_t opnorm_bound, uint32_t max_tries, const uint64_t* d_keys, size_t components, uint32_t domain,
                                        uint64_t index_base, void* stream) noexcept {
    return challenge_call("lsr_ntt_ring_challenge_batch_device", ctx, d_out, d_tries, count, kappa1, kappa2, opnorm_bound, max_tries, d_keys, components,
                          domain, index_base, true, stream);
}

}  // extern "C"
