// Scalar-weighted aggregation of ring vectors with an addend (batch.h "scalar-weighted aggregation of ring vectors"):
//   out[j][k] = addend[j][k] + sum_{i < terms} weights[j / components][k][i] v[j term_stride + i]   (scalars times ring vectors, mod q),
// the step that collapses the constraint families of a LaBRADOR / Greyhound-style argument by scalars psi and adds Pi^T w.  One streaming
// kernel per call in the context's arithmetic flavour; it reads q, the flavour's reduction constants and n, and no twiddle table: every
// context the library creates is served.  No workspace and no part in the context's ring ordering: the device form enqueues kernels in
// plain stream order and nothing else.
#include <algorithm>
#include <cstring>

#include "lambda_snark/batch.h"
#include "lsr_ring_call.hpp"
#include "lsr_ring_scalar_kernels.hpp"
#include "lsr_runtime.hpp"

namespace lsr {

static_assert(kScalarMaxSets == LSR_RING_SCALAR_COMBINE_MAX_SETS, "batch.h and the kernel agree on the sets of one call");
static_assert(kScalarThreads * 2 == LSR_RING_SCALAR_COMBINE_TILE, "batch.h documents the kernel's position tile");
static_assert(kScalarStage == LSR_RING_SCALAR_COMBINE_STAGE, "batch.h documents the weights the kernel stages at a time");
static_assert(kRingDotF64Period == LSR_RING_DOT_F64_RECENTRE_PERIOD, "batch.h documents the re-centring period");
static_assert((uint64_t)kScalarMaxSets * LSR_RING_DOT_MAX_TERMS <= (1ull << 20), "the weight words of one group are counted in 32 bits");

struct ScalarCombineCall {
    uint64_t len;             // width n
    uint64_t sets, terms, term_stride, components;
};

// vectors [first, first + count) of a call (vector `first` at d_out, d_status, d_addend and d_v); d_weights holds the groups from
// group_base on.  Plain stream order: one launch for the whole blocks of kScalarSetBlock sets and one for a ragged last block, each an
// instantiation for exactly its sets.  d_addend: NULL, or d_out itself, or a buffer apart from it.
static void scalar_combine_device(const NttContext& c, uint64_t* d_out, int32_t* d_status, const uint64_t* d_v, const uint64_t* d_weights,
                                  const uint64_t* d_addend, uint64_t first, uint64_t count, const ScalarCombineCall& call, uint64_t group_base,
                                  hipStream_t s) {
    // two positions per lane take 16-byte accesses: len = width n is even, so every vector is aligned when the buffers are
    const bool pairs = kScalarPositions == 2 && ((reinterpret_cast<uintptr_t>(d_out) | reinterpret_cast<uintptr_t>(d_v) | reinterpret_cast<uintptr_t>(d_addend)) & 15u) == 0;
    const uint64_t tile = kScalarThreads * (pairs ? 2 : 1);
    ScalarCombineJob job{};
    job.weights = d_weights;
    job.components = call.components;
    job.group_base = group_base;
    job.len = call.len;
    job.term_stride = call.term_stride;
    job.terms = static_cast<uint32_t>(call.terms);
    job.sets = static_cast<uint32_t>(call.sets);
    job.tiles = static_cast<uint32_t>((call.len + tile - 1) / tile);                     // len <= 2^32: at most 2^24
    const uint32_t whole = static_cast<uint32_t>(call.sets / kScalarSetBlock), ragged = static_cast<uint32_t>(call.sets % kScalarSetBlock);
    auto launch = [&](uint32_t set_first, uint32_t live, uint32_t set_blocks) {
        job.set_first = set_first;
        job.set_blocks = set_blocks;
        const uint64_t per_vector = (uint64_t)job.tiles * set_blocks;                    // at most 2^28
        // one launch covers at most 2^30 workgroups
        const uint64_t step = std::max<uint64_t>(1, (1ull << 30) / per_vector);
        for (uint64_t j0 = 0; j0 < count; j0 += step) {
            const uint64_t now = std::min(step, count - j0);
            job.out = d_out + j0 * call.sets * call.len;
            job.addend = d_addend ? d_addend + j0 * call.sets * call.len : nullptr;
            job.status = d_status + j0;
            job.v = d_v + j0 * call.term_stride * call.len;
            job.first = first + j0;
            const dim3 grid(static_cast<unsigned>(now * per_vector));
            for_flavour(c, [&](auto a) {
                for_tile_log<1, kScalarSetBlock>(static_cast<int>(live), [&](auto l) {
                    for_bool(pairs, [&](auto two) {
                        constexpr int P = decltype(two)::value ? kScalarPositions : 1;
                        hipLaunchKernelGGL((ring_scalar_combine_kernel<decltype(a), decltype(l)::value, P>), grid, dim3(kScalarThreads), 0, s, job, c.mod);
                    });
                });
            });
            LSR_HIP(hipGetLastError());
        }
    };
    if (whole) launch(0, kScalarSetBlock, whole);
    if (ragged) launch(whole * kScalarSetBlock, ragged, 1);
}

// Host buffers through bounded device chunks on the context's work stream.  While one output's operands fit the staging bound: chunks
// of whole outputs with the span of vectors they read (term_stride == 0: v goes up once) and their weight groups, the addend riding
// up in the output buffer (the device form's in-place addend).  Else one output at a time with its terms in groups: the weights of a
// group of terms are gathered from the [sets][terms] rows on the way up, and the in-place addend carries the running sum from one
// group to the next.  There the status is decided here, from the host's copy of the weights: a refused output runs no device work.
static void host_scalar_combine(const NttContext& c, uint64_t* out, int32_t* status, const uint64_t* v, const uint64_t* weights, const uint64_t* addend,
                                uint64_t count, const ScalarCombineCall& call) {
    const uint64_t len = call.len, sets = call.sets, terms = call.terms, ts = call.term_stride, per_group = sets * terms;
    const uint64_t fit = std::max<uint64_t>(1, (staging_bytes() / 8) / len);             // vectors of len words within the bound
    if (terms + sets <= fit) {
        // (chunk - 1) ts + terms vectors of v and chunk sets vectors of out within the bound
        const uint64_t chunk = std::min(count, (fit - terms + ts) / (ts + sets));
        host_staged(c, count, chunk,
                    {staged_items(v, nullptr, ts * len * 8, terms * len * 8), staged_groups(weights, per_group * 8, call.components),
                     staged_items(addend, out, sets * len * 8), staged_items(nullptr, status, 4)},
                    [&](const StagedChunk& k, hipStream_t s) {
                        uint64_t* const d_out = k.lane<uint64_t>(2);
                        scalar_combine_device(c, d_out, k.lane<int32_t>(3), k.lane<const uint64_t>(0), k.lane<const uint64_t>(1), addend ? d_out : nullptr,
                                              k.first, k.now, call, k.group_first, s);
                    });
        return;
    }
    DeviceGuard guard(c.device);
    std::lock_guard<std::mutex> lock(c.staging_mutex);   // serialises use of work_stream(c)
    hipStream_t s = work_stream(c);
    const uint64_t group_max = std::min(terms, fit > sets ? fit - sets : 1);
    DeviceBuffer<uint64_t> d_v(group_max * len), d_out(sets * len), d_weights(sets * group_max);
    DeviceBuffer<int32_t> d_status(1);
    for (uint64_t j = 0; j < count; ++j) {
        const uint64_t* const wg = weights + (j / call.components) * per_group;
        uint64_t* const o = out + j * sets * len;
        if (std::any_of(wg, wg + per_group, [&](uint64_t w) { return w >= c.modulus; })) {
            status[j] = -1;
            std::memset(o, 0, sets * len * 8);
            continue;
        }
        if (addend) LSR_HIP(hipMemcpyAsync(d_out.ptr, addend + j * sets * len, sets * len * 8, hipMemcpyHostToDevice, s));
        for (uint64_t i0 = 0; i0 < terms; i0 += group_max) {
            const uint64_t group = std::min(group_max, terms - i0);
            ScalarCombineCall part = call;
            part.terms = group;
            part.term_stride = 0;
            part.components = 1;
            LSR_HIP(hipMemcpyAsync(d_v.ptr, v + (j * ts + i0) * len, group * len * 8, hipMemcpyHostToDevice, s));
            LSR_HIP(hipMemcpy2DAsync(d_weights.ptr, group * 8, wg + i0, terms * 8, group * 8, sets, hipMemcpyHostToDevice, s));
            scalar_combine_device(c, d_out.ptr, d_status.ptr, d_v.ptr, d_weights.ptr, (addend || i0) ? d_out.ptr : nullptr, 0, 1, part, 0, s);
        }
        LSR_HIP(hipMemcpyAsync(o, d_out.ptr, sets * len * 8, hipMemcpyDeviceToHost, s));
        LSR_HIP(hipStreamSynchronize(s));
        status[j] = 1;
    }
}

}  // namespace lsr

// ------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------
namespace {

struct ScalarCounts {
    size_t vectors = 0, v_elems = 0, outputs = 0, out_elems = 0, weight_words = 0;   // (count - 1) term_stride + terms; times width; count sets; times width
};

// Argument checks that read no context (and never dereference ctx), in batch.h's order: -1 and a message, 1 for the empty call (a
// no-op), 0 to go on.
int scalar_combine_check(const char* where, const NttContext* ctx, const void* out, const void* status, const void* v, const void* weights, size_t count,
                         size_t sets, size_t terms, size_t ts, size_t width, size_t components, ScalarCounts& k) {
    if (!ctx || !out || !status || !v || !weights) return lsr::abi_refuse(where, "NULL context, out, status, v or weights");
    if (components == 0) return lsr::abi_refuse(where, "components must be at least 1");
    if (sets == 0 || sets > LSR_RING_SCALAR_COMBINE_MAX_SETS)
        return lsr::abi_refuse(where, "sets = " + std::to_string(sets) + " is not in 1 .. " + std::to_string(LSR_RING_SCALAR_COMBINE_MAX_SETS));
    if (terms == 0 || terms > LSR_RING_DOT_MAX_TERMS)
        return lsr::abi_refuse(where, "terms = " + std::to_string(terms) + " is not in 1 .. LSR_RING_DOT_MAX_TERMS (" + std::to_string(LSR_RING_DOT_MAX_TERMS) + ")");
    if (count == 0 || width == 0) return 1;
    // every product a shape takes, in ring elements (weights: in words) and then in bytes at the smallest ring (n = 2, 16 bytes)
    const size_t groups = (count - 1) / components + 1;
    size_t span = 0;
    const bool overflow = __builtin_mul_overflow(count - 1, ts, &span) || __builtin_add_overflow(span, terms, &k.vectors) ||
                          __builtin_mul_overflow(k.vectors, width, &k.v_elems) || __builtin_mul_overflow(count, sets, &k.outputs) ||
                          __builtin_mul_overflow(k.outputs, width, &k.out_elems) || __builtin_mul_overflow(groups, sets * terms, &k.weight_words) ||
                          __builtin_mul_overflow(k.vectors, (size_t)16, &span) || __builtin_mul_overflow(k.v_elems, (size_t)16, &span) ||
                          __builtin_mul_overflow(k.outputs, (size_t)16, &span) || __builtin_mul_overflow(k.out_elems, (size_t)16, &span) ||
                          __builtin_mul_overflow(k.weight_words, (size_t)16, &span);
    if (overflow) return lsr::abi_refuse(where, "the sizes of v, weights or out overflow size_t (count, sets, terms, term_stride, width, components)");
    return 0;
}

int scalar_combine_call(const char* where, const NttContext* ctx, uint64_t* out, int32_t* status, const uint64_t* v, const uint64_t* weights,
                        const uint64_t* addend, size_t count, size_t sets, size_t terms, size_t ts, size_t width, size_t components, bool device,
                        void* stream) noexcept {
    ScalarCounts k;
    const int rc = scalar_combine_check(where, ctx, out, status, v, weights, count, sets, terms, ts, width, components, k);
    if (rc != 0) return rc < 0 ? -1 : 0;
    return lsr::abi_guarded(where, [&] {
        size_t len = 0;
        if (__builtin_mul_overflow(width, (size_t)ctx->degree, &len)) throw std::runtime_error("width * n overflows size_t");
        if (len > (1ull << 32)) throw std::runtime_error("width * n = " + std::to_string(len) + " is above 2^32");
        const size_t elem_bytes = (size_t)ctx->degree * 8;
        size_t v_bytes = 0, out_bytes = 0;
        if (__builtin_mul_overflow(k.v_elems, elem_bytes, &v_bytes) || __builtin_mul_overflow(k.out_elems, elem_bytes, &out_bytes))
            throw std::runtime_error("the sizes of v or out overflow size_t at this ring degree");
        const char* const apart = ": the outputs must not share memory with an operand";
        lsr::require_apart(out, out_bytes, v, v_bytes, (std::string("out overlaps v") + apart).c_str());
        lsr::require_apart(out, out_bytes, weights, k.weight_words * 8, (std::string("out overlaps weights") + apart).c_str());
        lsr::require_apart(out, out_bytes, status, count * 4, "out overlaps status");
        if (addend && addend != out)
            lsr::require_apart(out, out_bytes, addend, out_bytes, "out overlaps addend without being equal to it: the in-place form takes addend == out exactly");
        lsr::require_device();
        // min(components, count): the same groups
        const lsr::ScalarCombineCall call{len, sets, terms, ts, std::min<uint64_t>(components, count)};
        if (device) {
            lsr::DeviceGuard guard(ctx->device);
            lsr::scalar_combine_device(*ctx, out, status, v, weights, addend, 0, count, call, 0, static_cast<hipStream_t>(stream));
        } else {
            lsr::host_scalar_combine(*ctx, out, status, v, weights, addend, count, call);
        }
    });
}

}  // namespace

extern "C" {

int lsr_ntt_ring_scalar_combine_batch(const NttContext* ctx, uint64_t* out, int32_t* status, const uint64_t* v, const uint64_t* weights,
                                      const uint64_t* addend, size_t count, size_t sets, size_t terms, size_t term_stride, size_t width,
                                      size_t components) noexcept {
    return scalar_combine_call("lsr_ntt_ring_scalar_combine_batch", ctx, out, status, v, weights, addend, count, sets, terms, term_stride, width,
                               components, false, nullptr);
}
int lsr_ntt_ring_scalar_combine_batch_device(const NttContext* ctx, uint64_t* d_out, int32_t* d_status, const uint64_t* d_v, const uint64_t* d_weights,
                                             const uint64_t* d_addend, size_t count, size_t sets, size_t terms, size_t term_stride, size_t width,
                                             size_t components, void* stream) noexcept {
    return scalar_combine_call("lsr_ntt_ring_scalar_combine_batch_device", ctx, d_out, d_status, d_v, d_weights, d_addend, count, sets, terms, term_stride,
                               width, components, true, stream);
}

}  // extern "C"
