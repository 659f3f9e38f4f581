// Batched fold of ring vectors by ring-valued challenges:
//   out[j][c] = sum_{i < terms} p[j][i] * v[j term_stride + i][c],   v: [vectors][width][n], p: [outputs][terms][n], out: [outputs][width][n].
// The transform of a challenge is shared by the `width` components of the vector it multiplies: terms + 1 + terms / width transforms
// per output polynomial instead of the 2 terms + 1 of a ring inner product on gathered operands, and no gathered temporaries.
//   n <= 4096: per chunk of outputs one launch_ntt of the chunk's challenges into the workspace (the b-hat rows of the ring inner
//              product) and ONE launch of ntt_tile_ring_fold, grid = (tiles of [width][n], outputs of the chunk).
//   n > 4096:  per chunk the strided forward rounds of the term vectors into the `wa` half of the workspace, launch_ntt of the
//              challenges into the `wb` half, the tile kernel as middle pass, one strided inverse round in place on out.
// The workspace is the ring inner product's (ring_dot_scratch, lsr_ring_workspace.hpp), under the same mutex and event.  What does not fit
// is taken in chunks of outputs, then of components, then in groups of terms with the raw accumulator waiting in `out` between
// launches (kRingDotFirst / kRingDotLast).
#include <algorithm>
#include <cstring>

#include "lambda_snark/batch.h"
#include "lsr_flavour.hpp"
#include "lsr_ring_call.hpp"
#include "lsr_ring_fold.hpp"
#include "lsr_ring_fold_kernels.hpp"
#include "lsr_ring_workspace.hpp"
#include "lsr_runtime.hpp"

namespace lsr {

constexpr size_t kFoldMaxGridY = 65535;

struct FoldOperands {
    uint64_t* c;
    const uint64_t *a, *bhat;
    size_t total;            // words of one output: width n
    uint32_t nterms;
    size_t a_term, a_out;    // words between consecutive terms / consecutive outputs' first terms
    uint32_t flags;
    size_t outputs;          // grid.y
};

template <class A, int LT, bool MID>
static void fold_tile(const NttContext& c, const FoldOperands& o, hipStream_t s) {
    const dim3 grid(static_cast<unsigned>((o.total + kTile - 1) / kTile), static_cast<unsigned>(o.outputs));
    hipLaunchKernelGGL((ntt_tile_ring_fold<A, LT, MID>), grid, dim3(kThreads), 0, s, o.c, o.a, o.bhat, o.total, o.nterms, o.a_term, o.a_out, o.flags, c.mod,
                       Flavour<A>::fwd(c), Flavour<A>::inv(c), Flavour<A>::consts(c));
}

template <class A, bool MID>
static void fold_tile_lt(const NttContext& c, int lt, const FoldOperands& o, hipStream_t s) {
    for_tile_log<MID ? 9 : 1, 12>(lt, [&](auto t) { fold_tile<A, decltype(t)::value, MID>(c, o, s); });
}

// first / last: this call starts / finishes the sums (the host variant stages long sums in groups of terms, as this function does)
template <class A>
static void ring_fold_enqueue(const NttContext& c, uint64_t* d_out, const uint64_t* d_v, const uint64_t* d_p, size_t outputs, size_t terms, size_t ts,
                              size_t width, bool first, bool last, hipStream_t s) {
    const size_t n = c.degree, polys = ring_dot_chunk_polys(c), vec = width * n;
    uint64_t* const ws = c.ring_dot_scratch.ptr;
    auto flags_of = [&](size_t i0, size_t group) { return ring_dot_flags(first && i0 == 0, last && i0 + group == terms); };
    if (c.logn <= kTileLog) {
        if (terms <= polys) {       // chunks of whole outputs: their challenges are contiguous in p
            const size_t chunk = std::min(polys / terms, kFoldMaxGridY);
            for (size_t j0 = 0; j0 < outputs; j0 += chunk) {
                const size_t now = std::min(chunk, outputs - j0);
                launch_ntt(c, ws, now * terms, false, s, nullptr, nullptr, d_p + j0 * terms * n);
                fold_tile_lt<A, false>(c, c.logn, {d_out + j0 * vec, d_v + j0 * ts * vec, ws, vec, (uint32_t)terms, vec, ts * vec, flags_of(0, terms), now}, s);
            }
            return;
        }
        for (size_t j = 0; j < outputs; ++j)
            for (size_t i0 = 0; i0 < terms; i0 += polys) {
                const size_t group = std::min(polys, terms - i0);
                launch_ntt(c, ws, group, false, s, nullptr, nullptr, d_p + (j * terms + i0) * n);
                fold_tile_lt<A, false>(c, c.logn, {d_out + j * vec, d_v + (j * ts + i0) * vec, ws, vec, (uint32_t)group, vec, 0, flags_of(i0, group), 1}, s);
            }
        return;
    }
    const int lt = mid_tile_log(c);
    uint64_t* const wa = ws;
    uint64_t* const wb = ws + polys * n;
    if (width <= polys && terms <= polys / width) {
        // whole outputs fit: chunks of outputs.  term_stride == 0: the forward rounds of v run once and serve every output;
        // term_stride == terms: the vectors of a chunk are contiguous, one launch; else one launch per output.
        const size_t chunk = std::min(polys / (terms * width), kFoldMaxGridY);
        const uint32_t flags = flags_of(0, terms);
        if (ts == 0) launch_strided_round(c, wa, d_v, terms * width, false, s);
        for (size_t j0 = 0; j0 < outputs; j0 += chunk) {
            const size_t now = std::min(chunk, outputs - j0);
            if (ts == terms) launch_strided_round(c, wa, d_v + j0 * ts * vec, now * terms * width, false, s);
            else if (ts != 0)
                for (size_t jj = 0; jj < now; ++jj) launch_strided_round(c, wa + jj * terms * vec, d_v + (j0 + jj) * ts * vec, terms * width, false, s);
            launch_ntt(c, wb, now * terms, false, s, nullptr, nullptr, d_p + j0 * terms * n);
            fold_tile_lt<A, true>(c, lt, {d_out + j0 * vec, wa, wb, vec, (uint32_t)terms, vec, ts == 0 ? 0 : terms * vec, flags, now}, s);
            if (flags & kRingDotLast) launch_strided_round(c, d_out + j0 * vec, nullptr, now * width, true, s);
        }
        return;
    }
    // one output at a time: its components in chunks, its terms in groups.  The whole width fits a group: the vectors of the group are
    // contiguous, one launch; else one launch per term.
    const size_t group_max = std::min(terms, polys), wmax = std::min(width, std::max<size_t>(1, polys / group_max));
    for (size_t j = 0; j < outputs; ++j)
        for (size_t c0 = 0; c0 < width; c0 += wmax) {
            const size_t wnow = std::min(wmax, width - c0);
            uint64_t* const out = d_out + j * vec + c0 * n;
            for (size_t i0 = 0; i0 < terms; i0 += group_max) {
                const size_t group = std::min(group_max, terms - i0);
                const uint32_t flags = flags_of(i0, group);
                const uint64_t* const from = d_v + (j * ts + i0) * vec + c0 * n;
                if (wnow == width) launch_strided_round(c, wa, from, group * width, false, s);
                else
                    for (size_t i = 0; i < group; ++i) launch_strided_round(c, wa + i * wnow * n, from + i * vec, wnow, false, s);
                launch_ntt(c, wb, group, false, s, nullptr, nullptr, d_p + (j * terms + i0) * n);
                fold_tile_lt<A, true>(c, lt, {out, wa, wb, wnow * n, (uint32_t)group, wnow * n, 0, flags, 1}, s);
                if (flags & kRingDotLast) launch_strided_round(c, out, nullptr, wnow, true, s);
            }
        }
}

// One call on the device (caller validated the arguments): workspace, ordering brackets, launches.
static void ring_fold_device(const NttContext& c, uint64_t* d_out, const uint64_t* d_v, const uint64_t* d_p, size_t outputs, size_t terms, size_t ts,
                             size_t width, hipStream_t s, bool first = true, bool last = true) {
    // the ring inner product's workspace, which every fold needs: the challenges are transformed into it at every n
    ring_call(c, c.ring_dot_scratch, ring_dot_scratch_words(c), true, s, [&] {
        for_flavour(c, [&](auto a) { ring_fold_enqueue<decltype(a)>(c, d_out, d_v, d_p, outputs, terms, ts, width, first, last, s); });
    });
}

// host buffers through bounded device chunks on the context's work stream: chunks of whole outputs (with the span of vectors they
// read) while one output's operands fit the staging bound, else one output at a time, its components in chunks and its terms in
// groups (the accumulator stays on the device between groups)
static void host_ring_fold(const NttContext& c, uint64_t* out, const uint64_t* v, const uint64_t* p, size_t outputs, size_t terms, size_t ts,
                           size_t width) {
    const size_t n = c.degree, vec = width * n;
    const size_t bound = std::max<size_t>(1, staging_bytes() / (n * 8));          // polynomials per staged operand
    if (width <= bound && terms <= bound / width) {
        const size_t fit_v = ts == 0 ? outputs : (bound / width - terms) / ts + 1;     // (now - 1) ts + terms vectors within the bound
        const size_t chunk = std::max<size_t>(1, std::min({outputs, fit_v, bound / terms, bound / width}));
        host_staged(c, outputs, chunk,
                    {staged_items(v, nullptr, ts * vec * 8, terms * vec * 8), staged_items(p, nullptr, terms * n * 8), staged_items(nullptr, out, vec * 8)},
                    [&](const StagedChunk& k, hipStream_t s) {
                        ring_fold_device(c, k.lane<uint64_t>(2), k.lane<const uint64_t>(0), k.lane<const uint64_t>(1), k.now, terms, ts, width, s);
                    });
        return;
    }
    DeviceGuard guard(c.device);
    std::lock_guard<std::mutex> lock(c.staging_mutex);   // serialises use of work_stream(c)
    hipStream_t s = work_stream(c);
    const size_t group_max = std::min(terms, bound), wmax = std::min(width, std::max<size_t>(1, bound / group_max));
    DeviceBuffer<uint64_t> dv(group_max * wmax * n), dp(group_max * n), dout(wmax * n);
    for (size_t j = 0; j < outputs; ++j)
        for (size_t c0 = 0; c0 < width; c0 += wmax) {
            const size_t wnow = std::min(wmax, width - c0);
            for (size_t i0 = 0; i0 < terms; i0 += group_max) {
                const size_t group = std::min(group_max, terms - i0);
                const uint64_t* const from = v + (j * ts + i0) * vec + c0 * n;
                if (wnow == width) LSR_HIP(hipMemcpyAsync(dv.ptr, from, group * vec * 8, hipMemcpyHostToDevice, s));
                else
                    for (size_t i = 0; i < group; ++i)
                        LSR_HIP(hipMemcpyAsync(dv.ptr + i * wnow * n, from + i * vec, wnow * n * 8, hipMemcpyHostToDevice, s));
                LSR_HIP(hipMemcpyAsync(dp.ptr, p + (j * terms + i0) * n, group * n * 8, hipMemcpyHostToDevice, s));
                ring_fold_device(c, dout.ptr, dv.ptr, dp.ptr, 1, group, 0, wnow, s, i0 == 0, i0 + group == terms);
            }
            LSR_HIP(hipMemcpyAsync(out + j * vec + c0 * n, dout.ptr, wnow * n * 8, hipMemcpyDeviceToHost, s));
            LSR_HIP(hipStreamSynchronize(s));
        }
}

}  // namespace lsr

// ------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------
namespace {

using lsr::FoldCounts;

// Argument checks that read no context (and never dereference ctx), in the documented order: -1 and a message, 1 for the empty call
// (a no-op), 0 to go on.
int ring_fold_check(const char* where, const NttContext* ctx, const void* out, const void* v, const void* p, size_t outputs, size_t terms,
                    size_t ts, size_t width, FoldCounts& k) {
    if (lsr::refuse_coeff_context(where, ctx)) return -1;
    if (!ctx || !out || !v || !p) return lsr::abi_refuse(where, "NULL context or buffer");
    return lsr::ring_fold_shape_check(where, outputs, terms, ts, width, k);
}

// The checks of a non-empty call that read the context, still before any device work.
void ring_fold_validate(const NttContext& ctx, const uint64_t* out, const uint64_t* v, const uint64_t* p, const FoldCounts& k) {
    lsr::refuse_above_two_pass(ctx, "ring fold on a context above n = 131072 is not supported (lsr_cyclic_ntt_context_create_large)");
    const size_t poly_bytes = (size_t)ctx.degree * 8;
    size_t bytes = 0;
    if (__builtin_mul_overflow(k.v_polys, poly_bytes, &bytes) || __builtin_mul_overflow(k.p_polys, poly_bytes, &bytes) ||
        __builtin_mul_overflow(k.out_polys, poly_bytes, &bytes))
        throw std::runtime_error("the sizes of v, p or out overflow size_t at this ring degree");
    lsr::require_apart(out, k.out_polys * poly_bytes, v, k.v_polys * poly_bytes, "out overlaps v: the output must not share memory with an operand");
    lsr::require_apart(out, k.out_polys * poly_bytes, p, k.p_polys * poly_bytes, "out overlaps p: the output must not share memory with an operand");
    lsr::require_device();
}

}  // namespace

extern "C" {

int lsr_ntt_ring_fold_batch(const NttContext* ctx, uint64_t* out, const uint64_t* v, const uint64_t* p, size_t outputs, size_t terms,
                            size_t term_stride, size_t width) noexcept {
    FoldCounts k;
    const int rc = ring_fold_check("lsr_ntt_ring_fold_batch", ctx, out, v, p, outputs, terms, term_stride, width, k);
    if (rc != 0) return rc < 0 ? -1 : 0;
    return lsr::abi_guarded("lsr_ntt_ring_fold_batch", [&] {
        ring_fold_validate(*ctx, out, v, p, k);
        lsr::host_ring_fold(*ctx, out, v, p, outputs, terms, term_stride, width);
    });
}

int lsr_ntt_ring_fold_batch_device(const NttContext* ctx, uint64_t* d_out, const uint64_t* d_v, const uint64_t* d_p, size_t outputs, size_t terms,
                                   size_t term_stride, size_t width, void* stream) noexcept {
    FoldCounts k;
    const int rc = ring_fold_check("lsr_ntt_ring_fold_batch_device", ctx, d_out, d_v, d_p, outputs, terms, term_stride, width, k);
    if (rc != 0) return rc < 0 ? -1 : 0;
    return lsr::abi_guarded("lsr_ntt_ring_fold_batch_device", [&] {
        ring_fold_validate(*ctx, d_out, d_v, d_p, k);
        lsr::DeviceGuard guard(ctx->device);
        lsr::ring_fold_device(*ctx, d_out, d_v, d_p, outputs, terms, term_stride, width, static_cast<hipStream_t>(stream));
    });
}

}  // extern "C"
