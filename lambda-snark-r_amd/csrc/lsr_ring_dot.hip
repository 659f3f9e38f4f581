// Batched ring inner product c_j = sum_{i < terms} a_{j,i} b_{j,i} in Z_q[X]/(X^n + 1) (negacyclic contexts) or Z_q[X]/(X^n - 1) (cyclic
// contexts): the rank-`terms` case of lsr_ring_mul.hip, with the products summed in registers and ONE inverse transform per output.
//   n <= 4096: ONE launch (ntt_tile_ring_dot): per output tile and term both forward transforms, the product added into a register
//              accumulator; the inverse after the last term — 16 terms + 8 bytes of HBM traffic per output residue.
//   n > 4096:  per chunk the strided forward rounds of the chunk's a and b terms into the workspace, the tile kernel as middle pass
//              (reads the raw tiles term by term, accumulates, runs its inverse rounds, writes raw elements to c), one strided inverse
//              round on c.
//   b_rows == 1 (one vector b for every output): b is transformed once per call (launch_ntt) into the workspace and the tile kernel
//              reads b-hat_i at its last-round positions instead of transforming b.
// The workspace holds a fixed number of polynomials (ring_dot_chunk_polys: a function of n and the process-wide chunk size).  More
// terms than fit are taken in groups, one launch sequence per group; between groups the raw accumulator waits in c
// (kRingDotFirst / kRingDotLast, lsr_ntt_kernels.hpp).
#include <algorithm>
#include <cstring>

#include "lambda_snark/batch.h"
#include "lsr_flavour.hpp"
#include "lsr_ntt_kernels.hpp"
#include "lsr_ring_call.hpp"
#include "lsr_ring_workspace.hpp"
#include "lsr_runtime.hpp"

static_assert(LSR_RING_DOT_F64_RECENTRE_PERIOD == (int)lsr::kRingDotF64Period, "batch.h documents the kernel's re-centring period");

namespace lsr {

// the terms (and, n <= 4096, terms n words of one output) are addressed through 32-bit buffer offsets: 4096 terms words stay below 2^31 bytes
static_assert((uint64_t)LSR_RING_DOT_MAX_TERMS * kTile * 8 <= (1ull << 31), "operand ranges of one tile must fit a buffer resource");

struct DotOperands {
    uint64_t* c;
    const uint64_t *a, *b;
    size_t total;        // words of c
    uint32_t nterms;
    size_t a_os, b_os;   // words between consecutive outputs' term-i polynomials
    uint32_t flags;
};

template <class A, int LT, bool MID, bool BHAT>
static void dot_tile(const NttContext& c, const DotOperands& o, hipStream_t s) {
    const unsigned grid = static_cast<unsigned>((o.total + kTile - 1) / kTile);
    hipLaunchKernelGGL((ntt_tile_ring_dot<A, LT, MID, BHAT>), dim3(grid), dim3(kThreads), 0, s, o.c, o.a, o.b, o.total, o.nterms, o.a_os, o.b_os, o.flags,
                       c.mod, Flavour<A>::fwd(c), Flavour<A>::inv(c), Flavour<A>::consts(c));
}

template <class A, bool MID, bool BHAT>
static void dot_tile_lt(const NttContext& c, int lt, const DotOperands& o, hipStream_t s) {
    for_tile_log<MID ? 9 : 1, 12>(lt, [&](auto t) { dot_tile<A, decltype(t)::value, MID, BHAT>(c, o, s); });
}

// (workspace sizing — ring_dot_chunk_polys, ring_dot_scratch_words: lsr_ring_workspace.hpp, shared with lsr_ring_fold.hip)

// first / last: this call starts / finishes the sums (the host variant stages long sums in groups of terms, as this function does)
template <class A>
static void ring_dot_enqueue(const NttContext& c, uint64_t* d_c, const uint64_t* d_a, const uint64_t* d_b, size_t batch, size_t terms, bool shared_b,
                             bool first, bool last, hipStream_t s) {
    const size_t n = c.degree, polys = ring_dot_chunk_polys(c);
    uint64_t* const ws = c.ring_dot_scratch.ptr;
    auto flags_of = [&](size_t i0, size_t group) { return ring_dot_flags(first && i0 == 0, last && i0 + group == terms); };
    if (c.logn <= kTileLog) {
        if (!shared_b) {
            dot_tile_lt<A, false, false>(c, c.logn, {d_c, d_a, d_b, batch * n, (uint32_t)terms, terms * n, terms * n, flags_of(0, terms)}, s);
            return;
        }
        for (size_t i0 = 0; i0 < terms; i0 += polys) {
            const size_t group = std::min(polys, terms - i0);
            launch_ntt(c, ws, group, false, s, nullptr, nullptr, d_b + i0 * n);
            dot_tile_lt<A, false, true>(c, c.logn, {d_c, d_a + i0 * n, ws, batch * n, (uint32_t)group, terms * n, 0, flags_of(i0, group)}, s);
        }
        return;
    }
    const int lt = mid_tile_log(c);
    uint64_t* const wa = ws;
    uint64_t* const wb = ws + polys * n;
    // all terms fit: chunks of whole outputs; else one output at a time, its terms in groups.  Either way the (output, term)
    // polynomials of one chunk and group are contiguous in a and b.
    const size_t group_max = std::min(terms, polys), chunk = group_max == terms ? polys / terms : 1;
    for (size_t i0 = 0; i0 < terms; i0 += group_max) {
        const size_t group = std::min(group_max, terms - i0);
        const uint32_t flags = flags_of(i0, group);
        if (shared_b) launch_ntt(c, wb, group, false, s, nullptr, nullptr, d_b + i0 * n);
        for (size_t j0 = 0; j0 < batch; j0 += chunk) {
            const size_t now = std::min(chunk, batch - j0), off = (j0 * terms + i0) * n;
            launch_strided_round(c, wa, d_a + off, now * group, false, s);
            if (!shared_b) launch_strided_round(c, wb, d_b + off, now * group, false, s);
            const DotOperands o{d_c + j0 * n, wa, wb, now * n, (uint32_t)group, group * n, group * n, flags};
            if (shared_b) dot_tile_lt<A, true, true>(c, lt, o, s);
            else dot_tile_lt<A, true, false>(c, lt, o, s);
            if (flags & kRingDotLast) launch_strided_round(c, d_c + j0 * n, nullptr, now, true, s);
        }
    }
}

// One call on the device (caller validated the arguments): workspace, ordering brackets, launches.
static void ring_dot_device(const NttContext& c, uint64_t* d_c, const uint64_t* d_a, const uint64_t* d_b, size_t batch, size_t terms, size_t b_rows,
                            hipStream_t s, bool first = true, bool last = true) {
    const bool shared_b = b_rows == 1 && batch > 1;
    ring_call(c, c.ring_dot_scratch, ring_dot_scratch_words(c), c.logn > kTileLog || shared_b, s, [&] {
        for_flavour(c, [&](auto a) { ring_dot_enqueue<decltype(a)>(c, d_c, d_a, d_b, batch, terms, shared_b, first, last, s); });
    });
}

// (host buffers: host_staged_dot, lsr_ring_call.hpp)
static void host_ring_dot(const NttContext& c, uint64_t* out, const uint64_t* a, const uint64_t* b, size_t batch, size_t terms, size_t b_rows) {
    host_staged_dot(c, out, a, b, batch, terms, b_rows,
                    [&](uint64_t* d_c, const uint64_t* d_a, const uint64_t* d_b, size_t now, size_t group, size_t rows, hipStream_t s, bool first, bool last) {
                        ring_dot_device(c, d_c, d_a, d_b, now, group, rows, s, first, last);
                    });
}

}  // namespace lsr

// ------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------
// Argument checks that need no device (and no dereference of ctx), in the documented order: -1 and a message, or 0 to go on.
static int ring_dot_check(const char* where, const NttContext* ctx, const void* c, const void* a, const void* b, size_t batch, size_t terms,
                          size_t b_rows) {
    if (lsr::refuse_coeff_context(where, ctx)) return -1;
    if (!ctx || !c || !a || !b) return lsr::abi_refuse(where, "NULL context or buffer");
    if (b_rows != 1 && b_rows != batch)
        return lsr::abi_refuse(where, "b_rows must be 1 or batch (" + std::to_string(batch) + "), got " + std::to_string(b_rows));
    if (terms == 0) return lsr::abi_refuse(where, "terms must be at least 1");
    return 0;
}

// The checks of a non-empty call that read the context, still before any device work.
static void ring_dot_validate(const NttContext& ctx, const uint64_t* c, const uint64_t* a, const uint64_t* b, size_t batch, size_t terms, size_t b_rows) {
    lsr::refuse_above_two_pass(ctx, "ring inner product on a context above n = 131072 is not supported (lsr_cyclic_ntt_context_create_large)");
    if (terms > LSR_RING_DOT_MAX_TERMS)
        throw std::runtime_error("terms = " + std::to_string(terms) + " is above LSR_RING_DOT_MAX_TERMS (" + std::to_string(LSR_RING_DOT_MAX_TERMS) + ")");
    const size_t poly_bytes = (size_t)ctx.degree * 8;
    lsr::require_apart(c, batch * poly_bytes, a, batch * terms * poly_bytes, "c overlaps a: the output must not share memory with an operand");
    lsr::require_apart(c, batch * poly_bytes, b, b_rows * terms * poly_bytes, "c overlaps b: the output must not share memory with an operand");
}

extern "C" {

int lsr_ntt_ring_dot_batch(const NttContext* ctx, uint64_t* c, const uint64_t* a, const uint64_t* b, size_t batch, size_t terms,
                           size_t b_rows) noexcept {
    if (ring_dot_check("lsr_ntt_ring_dot_batch", ctx, c, a, b, batch, terms, b_rows) != 0) return -1;
    if (batch == 0) return 0;
    return lsr::abi_guarded("lsr_ntt_ring_dot_batch", [&] {
        ring_dot_validate(*ctx, c, a, b, batch, terms, b_rows);
        lsr::require_device();
        lsr::host_ring_dot(*ctx, c, a, b, batch, terms, b_rows);
    });
}

int lsr_ntt_ring_dot_batch_device(const NttContext* ctx, uint64_t* d_c, const uint64_t* d_a, const uint64_t* d_b, size_t batch, size_t terms,
                                  size_t b_rows, void* stream) noexcept {
    if (ring_dot_check("lsr_ntt_ring_dot_batch_device", ctx, d_c, d_a, d_b, batch, terms, b_rows) != 0) return -1;
    if (batch == 0) return 0;
    return lsr::abi_guarded("lsr_ntt_ring_dot_batch_device", [&] {
        ring_dot_validate(*ctx, d_c, d_a, d_b, batch, terms, b_rows);
        lsr::require_device();
        lsr::DeviceGuard guard(ctx->device);
        lsr::ring_dot_device(*ctx, d_c, d_a, d_b, batch, terms, b_rows, static_cast<hipStream_t>(stream));
    });
}

}  // extern "C"
