// Seeded ring sampling on the device and seed-expanded ring matrices (batch.h "seeded ring sampling"): UNIFORM, BOUNDED
// and BALL elements of the context's ring from ChaCha20 streams whose keys may be device-resident transcript digests, and the resident
// matrix of lsr_ring_matvec.hip sampled straight into its handle.  Integer code that reads only q and n of the context: one path for
// every flavour, every ring degree and both rings.  The device form enqueues kernels and nothing else.
#include <algorithm>

#include "lambda_snark/batch.h"
#include "lsr_keys.hpp"
#include "lsr_ring_call.hpp"
#include "lsr_ring_matrix.hpp"
#include "lsr_ring_sample_kernels.hpp"
#include "lsr_runtime.hpp"

namespace lsr {

static_assert(kRingSampleMaxWords == LSR_RING_SAMPLE_MAX_WORDS, "batch.h and the kernels agree on the attempt cap");
static_assert(kBallLdsMaxLog == kTwoPassMaxLog2, "the LDS form of BALL serves every two-pass context");
// word indices stay below 64 n <= 2^28 on the largest context (n = 2^22): the 32-bit block counter never wraps
static_assert(LSR_RING_SAMPLE_MAX_WORDS == 64, "64 n <= 2^28");

struct SampleCall {
    int kind;
    uint64_t param;
    uint64_t components;      // min(components, count): the same streams, and the kernels' 32-bit division applies more often
    uint32_t domain;
    uint64_t index_base;
};

static unsigned bit_length(uint64_t v) { return v ? 64u - (unsigned)__builtin_clzll(v) : 0u; }

// elements [first, first + count) of a call into d_out (element `first` at d_out); d_keys holds the key groups from group_base on.
// The ring is given by its modulus and degree alone: any q >= 2, prime or not (the ring handles of lsr_ring_mod_matvec.hip sample
// under a modulus no context has).
struct SampleRing {
    uint64_t modulus;
    int logn;
    uint32_t degree;
};
static void sample_device(const SampleRing& c, uint64_t* d_out, uint64_t first, uint64_t count, const SampleCall& call, const uint64_t* d_keys,
                          uint64_t group_base, hipStream_t s) {
    if (call.kind == LSR_RING_SAMPLE_BALL) {
        RingBallJob job{d_out, d_keys, call.index_base, call.components, group_base, first, count, c.modulus, (uint32_t)call.param, call.domain, (uint32_t)c.logn};
        const bool lds = c.logn <= kBallLdsMaxLog;
        const uint32_t chunk = std::min<uint32_t>(((uint32_t)call.param + 7u) & ~7u, kBallChunkWords);
        const size_t bytes = (size_t)chunk * 8 + (lds ? std::max<size_t>(1, ((size_t)c.degree + 15) / 16) * 4 : 0);
        const unsigned grid = static_cast<unsigned>(std::min<uint64_t>(count, 1u << 20));
        if (lds) hipLaunchKernelGGL(ring_sample_ball_kernel<true>, dim3(grid), dim3(kRingSampleThreads), bytes, s, job);
        else hipLaunchKernelGGL(ring_sample_ball_kernel<false>, dim3(grid), dim3(kRingSampleThreads), bytes, s, job);
        LSR_HIP(hipGetLastError());
        return;
    }
    const uint64_t beta = call.kind == LSR_RING_SAMPLE_BOUNDED ? call.param : 0;
    const uint64_t m = call.kind == LSR_RING_SAMPLE_BOUNDED ? 2 * beta + 1 : c.modulus;     // beta <= (q - 1) / 2: no overflow
    const unsigned width = bit_length(m - 1);
    RingSampleJob job{};
    job.keys = d_keys;
    job.index_base = call.index_base;
    job.components = call.components;
    job.group_base = group_base;
    job.q = c.modulus;
    job.m = m;
    job.beta = beta;
    job.mask = width == 64 ? ~0ull : (1ull << width) - 1;
    job.width = width;
    job.fields = 64 / width;
    job.domain = call.domain;
    job.logn = (uint32_t)c.logn;
    // one launch covers at most 2^30 workgroups
    const uint64_t lanes_per_element = c.logn >= 3 ? (uint64_t)c.degree >> 3 : 1;
    const uint64_t step = std::max<uint64_t>(1, ((1ull << 30) * kRingSampleThreads) / lanes_per_element);
    for (uint64_t e0 = 0; e0 < count; e0 += step) {
        job.out = d_out + (e0 << c.logn);
        job.first = first + e0;
        job.count = std::min(step, count - e0);
        const unsigned grid = static_cast<unsigned>((job.count * lanes_per_element + kRingSampleThreads - 1) / kRingSampleThreads);
        if (c.logn >= 3) hipLaunchKernelGGL(ring_sample_kernel, dim3(grid), dim3(kRingSampleThreads), 0, s, job);
        else hipLaunchKernelGGL(ring_sample_small_kernel, dim3(grid), dim3(kRingSampleThreads), 0, s, job);
        LSR_HIP(hipGetLastError());
    }
}

static void sample_device(const NttContext& c, uint64_t* d_out, uint64_t first, uint64_t count, const SampleCall& call, const uint64_t* d_keys,
                          uint64_t group_base, hipStream_t s) {
    sample_device(SampleRing{c.modulus, c.logn, c.degree}, d_out, first, count, call, d_keys, group_base, s);
}

void sample_uniform_device(uint64_t q, int logn, uint64_t* d_out, uint64_t count, const uint64_t* d_key, uint32_t domain, uint64_t index_base,
                           hipStream_t s) {
    sample_device(SampleRing{q, logn, 1u << logn}, d_out, 0, count, SampleCall{LSR_RING_SAMPLE_UNIFORM, 0, count, domain, index_base}, d_key, 0, s);
}

}  // namespace lsr

// ------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------
static int sample_call(const char* where, const NttContext* ctx, uint64_t* out, size_t count, int kind, uint64_t param, const uint64_t* keys,
                       size_t components, uint32_t domain, uint64_t index_base, bool device, void* stream) noexcept {
    // (1) reads nothing, (2) reads no handle, (3) reads q and n of the context
    if (!ctx || !out || !keys) return lsr::abi_refuse(where, "NULL context, buffer or keys");
    if (kind != LSR_RING_SAMPLE_UNIFORM && kind != LSR_RING_SAMPLE_BOUNDED && kind != LSR_RING_SAMPLE_BALL)
        return lsr::abi_refuse(where, "kind = " + std::to_string(kind) + " is none of LSR_RING_SAMPLE_UNIFORM, _BOUNDED, _BALL");
    if (components == 0) return lsr::abi_refuse(where, "components must be at least 1");
    if (kind == LSR_RING_SAMPLE_UNIFORM && param != 0) return lsr::abi_refuse(where, "UNIFORM takes param = 0, not " + std::to_string(param));
    if (kind == LSR_RING_SAMPLE_BOUNDED && (param == 0 || param > (ctx->modulus - 1) / 2))
        return lsr::abi_refuse(where, "BOUNDED takes 1 <= beta <= (q - 1) / 2 = " + std::to_string((ctx->modulus - 1) / 2) + ", not " + std::to_string(param));
    if (kind == LSR_RING_SAMPLE_BALL && (param == 0 || param > ctx->degree))
        return lsr::abi_refuse(where, "BALL takes 1 <= kappa <= n = " + std::to_string(ctx->degree) + ", not " + std::to_string(param));
    if (count == 0) return 0;
    return lsr::abi_guarded(where, [&] {
        if (index_base + components < index_base) throw std::runtime_error("index_base + components overflows 64 bits");
        lsr::require_device();
        const lsr::SampleCall call{kind, param, std::min<uint64_t>(components, count), domain, index_base};
        if (device) {
            lsr::DeviceGuard guard(ctx->device);
            lsr::sample_device(*ctx, out, 0, count, call, keys, 0, static_cast<hipStream_t>(stream));
        } else {
            // host buffers through bounded device chunks of whole elements; each chunk brings its own key groups
            lsr::host_staged(*ctx, count, lsr::staging_chunk(count, ctx->degree),
                             {lsr::staged_groups(keys, 32, call.components), lsr::staged_items(nullptr, out, (size_t)ctx->degree * 8)},
                             [&](const lsr::StagedChunk& k, hipStream_t s) {
                                 lsr::sample_device(*ctx, k.lane<uint64_t>(1), k.first, k.now, call, k.lane<const uint64_t>(0), k.group_first, s);
                             });
        }
    });
}

extern "C" {

void lsr_ring_sample_key_from_seed(uint64_t seed, uint64_t key[4]) noexcept {
    if (key) lsr::key_words(lsr::expand_seed64(seed), key);
}

int lsr_ntt_ring_sample_batch(const NttContext* ctx, uint64_t* out, size_t count, int kind, uint64_t param, const uint64_t* keys, size_t components,
                              uint32_t domain, uint64_t index_base) noexcept {
    return sample_call("lsr_ntt_ring_sample_batch", ctx, out, count, kind, param, keys, components, domain, index_base, false, nullptr);
}

int lsr_ntt_ring_sample_batch_device(const NttContext* ctx, uint64_t* d_out, size_t count, int kind, uint64_t param, const uint64_t* d_keys,
                                     size_t components, uint32_t domain, uint64_t index_base, void* stream) noexcept {
    return sample_call("lsr_ntt_ring_sample_batch_device", ctx, d_out, count, kind, param, d_keys, components, domain, index_base, true, stream);
}

LsrRingMatrix* lsr_ntt_ring_matrix_create_seeded(const NttContext* ctx, const uint64_t key[4], uint32_t domain, uint64_t index_base, size_t rows,
                                                 size_t cols) noexcept {
    // (rows * cols is within the caps when either functor runs)
    lsr::DeviceBuffer<uint64_t> d_key;
    LsrRingMatrix* mat = lsr::matrix_create_filled(
        "lsr_ntt_ring_matrix_create_seeded", ctx, key, rows, cols,
        [&] {
            if (index_base + rows * cols < index_base) throw std::runtime_error("index_base + rows * cols overflows 64 bits");
        },
        [&](uint64_t* d_m, hipStream_t s) {
            d_key.allocate(4);
            LSR_HIP(hipMemcpyAsync(d_key.ptr, key, 32, hipMemcpyHostToDevice, s));
            const lsr::SampleCall call{LSR_RING_SAMPLE_UNIFORM, 0, rows * cols, domain, index_base};
            lsr::sample_device(*ctx, d_m, 0, rows * cols, call, d_key.ptr, 0, s);
        });
    // (the create synchronised its stream: the key is no longer read)
    if (d_key.ptr) {
        try {
            lsr::DeviceGuard guard(ctx->device);
            d_key.release();
        } catch (...) {
            d_key.release();
        }
    }
    return mat;
}

}  // extern "C"
