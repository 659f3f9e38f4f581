// Bit-packed encoding and decoding of short ring elements (batch.h "bit-packed ring elements"): the bytes of a proof
// message — gadget digits, folded witnesses, ternary and BALL elements, uniform elements — from device-resident vectors and back,
// with a status that tells a verifier a non-canonical encoding before anything derived from it enters Fiat–Shamir.  Integer kernels
// that read q and n of a context and nothing else: every context the library creates is served.  No workspace and no part in the
// context's ring ordering: the device forms enqueue kernels in plain stream order and nothing else.
#include <algorithm>

#include "lambda_snark/batch.h"
#include "lsr_ring_call.hpp"
#include "lsr_ring_pack_kernels.hpp"
#include "lsr_runtime.hpp"

namespace lsr {

static_assert(kPackCentred == LSR_RING_PACK_CENTRED && kPackResidue == LSR_RING_PACK_RESIDUE, "batch.h and the kernels agree on the modes");
static_assert(kPackThreads * 2 == LSR_RING_PACK_TILE, "batch.h documents the kernels' tile");

struct PackCall {
    uint64_t n, wpe;          // ring degree; W
    int mode;
    unsigned bits;
};

static PackJob pack_job(const NttContext& c, uint64_t* d_words, uint64_t* d_x, int32_t* d_status, uint64_t count, const PackCall& call) {
    PackJob job{};
    job.words = d_words;
    job.x = d_x;
    job.status = d_status;
    job.q = c.modulus;
    job.half = (c.modulus - 1) / 2;
    job.total = count * call.n;
    job.count = count;
    job.logn = static_cast<uint32_t>(__builtin_ctzll(call.n));
    job.bits = call.bits;
    job.wpe = static_cast<uint32_t>(call.wpe);               // n <= 2^22: below 2^22
    return job;
}

// `blocks` workgroups as launches of at most 2^30, each told where it starts (job.tile_base in units of `per_block`)
template <class Launch>
static void pack_launches(PackJob& job, uint64_t blocks, uint64_t per_block, Launch&& launch) {
    for (uint64_t b0 = 0; b0 < blocks; b0 += 1ull << 30) {
        job.tile_base = b0 * per_block;
        launch(dim3(static_cast<unsigned>(std::min<uint64_t>(1ull << 30, blocks - b0))));
        LSR_HIP(hipGetLastError());
    }
}

// the statuses of elements that span workgroups start at 1 (a kernel: a captured hipMemsetAsync ran on the first replay only)
static void pack_fill_status(int32_t* d_status, uint64_t count, uint64_t n, int p, hipStream_t s) {
    if (n <= (uint64_t)kPackThreads * p) return;
    for (uint64_t e0 = 0; e0 < count; e0 += (1ull << 30) * kPackThreads) {
        const uint64_t now = std::min<uint64_t>((1ull << 30) * kPackThreads, count - e0);
        hipLaunchKernelGGL(ring_pack_fill_status_kernel, dim3(static_cast<unsigned>((now + kPackThreads - 1) / kPackThreads)), dim3(kPackThreads), 0, s,
                           d_status + e0, now);
        LSR_HIP(hipGetLastError());
    }
}

static void pack_device(const NttContext& c, uint64_t* d_out, int32_t* d_status, const uint64_t* d_x, uint64_t count, const PackCall& call, hipStream_t s) {
    PackJob job = pack_job(c, d_out, const_cast<uint64_t*>(d_x), d_status, count, call);
    if (call.n < 64) {
        pack_launches(job, (count + kPackThreads - 1) / kPackThreads, kPackThreads, [&](dim3 grid) {
            for_bool(call.mode == kPackCentred, [&](auto centred) {
                constexpr int M = decltype(centred)::value ? kPackCentred : kPackResidue;
                hipLaunchKernelGGL((ring_pack_small_kernel<M>), grid, dim3(kPackThreads), 0, s, job);
            });
        });
        return;
    }
    const bool pairs = (reinterpret_cast<uintptr_t>(d_x) & 15u) == 0;        // n is even: every element is aligned when the buffer is
    const uint64_t tile = kPackThreads * (pairs ? 2 : 1);
    pack_fill_status(d_status, count, call.n, pairs ? 2 : 1, s);
    pack_launches(job, (job.total + tile - 1) / tile, 1, [&](dim3 grid) {
        for_bool(pairs, [&](auto two) {
            for_bool(call.mode == kPackCentred, [&](auto centred) {
                constexpr int P = decltype(two)::value ? 2 : 1, M = decltype(centred)::value ? kPackCentred : kPackResidue;
                hipLaunchKernelGGL((ring_pack_kernel<P, M>), grid, dim3(kPackThreads), 0, s, job);
            });
        });
    });
}

static void unpack_device(const NttContext& c, uint64_t* d_out, int32_t* d_status, const uint64_t* d_in, uint64_t count, const PackCall& call, hipStream_t s) {
    PackJob job = pack_job(c, const_cast<uint64_t*>(d_in), d_out, d_status, count, call);
    const bool pairs = (reinterpret_cast<uintptr_t>(d_out) & 15u) == 0;
    const uint64_t tile = kPackThreads * (pairs ? 2 : 1);
    pack_fill_status(d_status, count, call.n, pairs ? 2 : 1, s);
    pack_launches(job, (job.total + tile - 1) / tile, 1, [&](dim3 grid) {
        for_bool(pairs, [&](auto two) {
            for_bool(call.mode == kPackCentred, [&](auto centred) {
                constexpr int P = decltype(two)::value ? 2 : 1, M = decltype(centred)::value ? kPackCentred : kPackResidue;
                if (call.n < 64) hipLaunchKernelGGL((ring_unpack_direct_kernel<P, M>), grid, dim3(kPackThreads), 0, s, job);
                else hipLaunchKernelGGL((ring_unpack_kernel<P, M>), grid, dim3(kPackThreads), 0, s, job);
            });
        });
    });
}

// Host buffers through bounded device chunks of whole elements on the context's work stream: `in_words` words per element go up,
// `out_words` words and a status come back.
static void host_pack(const NttContext& c, uint64_t* out, int32_t* status, const uint64_t* in, uint64_t count, const PackCall& call, bool unpack) {
    const uint64_t in_words = unpack ? call.wpe : call.n, out_words = unpack ? call.n : call.wpe;
    host_staged(c, count, staging_chunk(count, in_words + out_words),
                {staged_items(in, nullptr, in_words * 8), staged_items(nullptr, out, out_words * 8), staged_items(nullptr, status, 4)},
                [&](const StagedChunk& k, hipStream_t s) {
                    if (unpack) unpack_device(c, k.lane<uint64_t>(1), k.lane<int32_t>(2), k.lane<const uint64_t>(0), k.now, call, s);
                    else pack_device(c, k.lane<uint64_t>(1), k.lane<int32_t>(2), k.lane<const uint64_t>(0), k.now, call, s);
                });
}

}  // namespace lsr

// ------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------
namespace {

unsigned bit_length(uint64_t v) { return v ? 64u - static_cast<unsigned>(__builtin_clzll(v)) : 0u; }

int pack_call(const char* where, const NttContext* ctx, uint64_t* out, int32_t* status, const uint64_t* in, size_t count, int mode, unsigned bits,
              bool unpack, bool device, void* stream) noexcept {
    if (!ctx || !out || !status || !in) return lsr::abi_refuse(where, unpack ? "NULL context, out, status or in" : "NULL context, out, status or x");
    if (mode != LSR_RING_PACK_CENTRED && mode != LSR_RING_PACK_RESIDUE)
        return lsr::abi_refuse(where, "mode = " + std::to_string(mode) + " is neither LSR_RING_PACK_CENTRED nor LSR_RING_PACK_RESIDUE");
    if (bits < 1 || bits > 63) return lsr::abi_refuse(where, "bits = " + std::to_string(bits) + " is not in 1 .. 63");
    if (count == 0) return 0;
    // the sizes read the context's degree and nothing else
    const size_t n = ctx->degree, wpe = lsr_ring_pack_words(ctx->degree, bits);
    size_t elems = 0, words = 0, bytes = 0;
    if (__builtin_mul_overflow(count, n, &elems) || __builtin_mul_overflow(count, wpe, &words) || __builtin_mul_overflow(elems, (size_t)8, &bytes) ||
        __builtin_mul_overflow(words, (size_t)8, &bytes))
        return lsr::abi_refuse(where, "count * n or count * W overflows size_t");
    return lsr::abi_guarded(where, [&] {
        const size_t out_bytes = (unpack ? elems : words) * 8, in_bytes = (unpack ? words : elems) * 8;
        lsr::require_apart(out, out_bytes, in, in_bytes, unpack ? "out overlaps in" : "out overlaps x");
        lsr::require_apart(out, out_bytes, status, count * 4, "out overlaps status");
        lsr::require_apart(status, count * 4, in, in_bytes, unpack ? "status overlaps in" : "status overlaps x");
        if (((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(in)) & 7u) != 0 || (reinterpret_cast<uintptr_t>(status) & 3u) != 0)
            throw std::runtime_error("the word buffers must be 8-byte aligned and status 4-byte aligned");
        lsr::require_device();
        if (n < 2 || (n & (n - 1)) != 0) throw std::runtime_error("the context's degree is not a power of two");
        const lsr::PackCall call{n, wpe, mode, bits};
        if (device) {
            lsr::DeviceGuard guard(ctx->device);
            if (unpack) lsr::unpack_device(*ctx, out, status, in, count, call, static_cast<hipStream_t>(stream));
            else lsr::pack_device(*ctx, out, status, in, count, call, static_cast<hipStream_t>(stream));
        } else {
            lsr::host_pack(*ctx, out, status, in, count, call, unpack);
        }
    });
}

}  // namespace

extern "C" {

size_t lsr_ring_pack_words(uint32_t n, unsigned bits) noexcept {
    if (bits < 1 || bits > 63) return 0;
    return static_cast<size_t>(((uint64_t)n * bits + 63) / 64);
}

unsigned lsr_ring_pack_min_bits(uint64_t q, int mode, uint64_t bound) noexcept {
    if (q == 0 || bound == 0) return 0;
    unsigned bits = 0;
    if (mode == LSR_RING_PACK_CENTRED) {
        if (bound > (q - 1) / 2) return 0;
        bits = bit_length(bound) + 1;
    } else if (mode == LSR_RING_PACK_RESIDUE) {
        if (bound > q - 1) return 0;
        bits = bit_length(bound);
    }
    return bits > 63 ? 0 : bits;
}

int lsr_ntt_ring_pack_batch(const NttContext* ctx, uint64_t* out, int32_t* status, const uint64_t* x, size_t count, int mode, unsigned bits) noexcept {
    return pack_call("lsr_ntt_ring_pack_batch", ctx, out, status, x, count, mode, bits, false, false, nullptr);
}
int lsr_ntt_ring_pack_batch_device(const NttContext* ctx, uint64_t* d_out, int32_t* d_status, const uint64_t* d_x, size_t count, int mode, unsigned bits,
                                   void* stream) noexcept {
    return pack_call("lsr_ntt_ring_pack_batch_device", ctx, d_out, d_status, d_x, count, mode, bits, false, true, stream);
}
int lsr_ntt_ring_unpack_batch(const NttContext* ctx, uint64_t* out, int32_t* status, const uint64_t* in, size_t count, int mode, unsigned bits) noexcept {
    return pack_call("lsr_ntt_ring_unpack_batch", ctx, out, status, in, count, mode, bits, true, false, nullptr);
}
int lsr_ntt_ring_unpack_batch_device(const NttContext* ctx, uint64_t* d_out, int32_t* d_status, const uint64_t* d_in, size_t count, int mode,
                                     unsigned bits, void* stream) noexcept {
    return pack_call("lsr_ntt_ring_unpack_batch_device", ctx, d_out, d_status, d_in, count, mode, bits, true, true, stream);
}

}  // extern "C"
