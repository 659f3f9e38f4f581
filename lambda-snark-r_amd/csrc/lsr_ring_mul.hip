// Batched ring multiply c = a b in Z_q[X]/(X^n + 1) (negacyclic contexts) or Z_q[X]/(X^n - 1) (cyclic contexts): the composition
// forward, forward, pointwise product, inverse that the reference leaves to its caller (cpp-core/src/ntt.cpp:106-119), fused.
//   n <= 4096: ONE launch (ntt_tile_ring_mul): per tile both forward transforms, the product in registers, the inverse — 24 bytes
//              of HBM traffic per output residue (read a, read b, write c).
//   n > 4096:  per chunk of the batch the two-pass schedule with the product in the middle pass — strided forward round of b into the
//              workspace, strided forward round of a into c, the tile kernel as middle pass (both tiles forward, product, inverse, in
//              place in c), strided inverse round on c: 9 polynomial passes instead of the composed sequence's 15-19.
//   b_rows == 1 (one b for every product): b is transformed once per call (launch_ntt) and the tile kernel reads b-hat at its
//              last-round positions instead of transforming b.
#include <algorithm>
#include <cstring>

#include "lambda_snark/batch.h"
#include "lsr_flavour.hpp"
#include "lsr_ntt_kernels.hpp"
#include "lsr_ring_call.hpp"
#include "lsr_runtime.hpp"

namespace lsr {

template <class A, int LT, bool MID, bool BHAT>
static void ring_tile(const NttContext& c, uint64_t* d_c, const uint64_t* d_a, const uint64_t* d_b, size_t total, hipStream_t s) {
    const unsigned grid = static_cast<unsigned>((total + kTile - 1) / kTile);
    hipLaunchKernelGGL((ntt_tile_ring_mul<A, LT, MID, BHAT>), dim3(grid), dim3(kThreads), 0, s, d_c, d_a, d_b, total, c.mod, Flavour<A>::fwd(c),
                       Flavour<A>::inv(c), Flavour<A>::consts(c));
}

template <class A, bool MID, bool BHAT>
static void ring_tile_lt(const NttContext& c, int lt, uint64_t* d_c, const uint64_t* d_a, const uint64_t* d_b, size_t total, hipStream_t s) {
    for_tile_log<MID ? 9 : 1, 12>(lt, [&](auto t) { ring_tile<A, decltype(t)::value, MID, BHAT>(c, d_c, d_a, d_b, total, s); });
}

// Polynomials per chunk of an n > 4096 product: two arrays are live between passes (the c chunk and the workspace chunk), so each
// gets half of the Infinity Cache budget of a two-pass transform (ntt_chunk_bytes(): 256 MiB -> 128 MiB each, 256 polynomials at
// n = 2^16, 128 at n = 2^17).
static size_t ring_chunk_polys(const NttContext& c) { return std::max<size_t>(1, (ntt_chunk_bytes() / 2) >> (c.logn + 3)); }
// Workspace words: n > 4096 — one chunk of transformed b plus one b-hat row; n <= 4096 — one b-hat row.  A function of n (and of the
// process-wide chunk size) only, never of the batch.
static size_t ring_scratch_words(const NttContext& c) {
    const size_t n = c.degree;
    return c.logn > kTileLog ? ring_chunk_polys(c) * n + n : n;
}

template <class A>
static void ring_mul_enqueue(const NttContext& c, uint64_t* d_c, const uint64_t* d_a, const uint64_t* d_b, size_t batch, bool shared_b, hipStream_t s) {
    const size_t n = c.degree;
    uint64_t* const ws = c.ring_scratch.ptr;
    if (c.logn <= kTileLog) {
        if (shared_b) {
            launch_ntt(c, ws, 1, false, s, nullptr, nullptr, d_b);
            ring_tile_lt<A, false, true>(c, c.logn, d_c, d_a, ws, batch * n, s);
        } else {
            ring_tile_lt<A, false, false>(c, c.logn, d_c, d_a, d_b, batch * n, s);
        }
        return;
    }
    const int lt = mid_tile_log(c);
    const size_t chunk = ring_chunk_polys(c);
    uint64_t* const b_hat = ws + chunk * n;
    if (shared_b) launch_ntt(c, b_hat, 1, false, s, nullptr, nullptr, d_b);
    for (size_t first = 0; first < batch; first += chunk) {
        const size_t now = std::min(chunk, batch - first), off = first * n;
        uint64_t* const cc = d_c + off;
        const uint64_t* const ac = d_a + off;
        if (!shared_b) launch_strided_round(c, ws, d_b + off, now, false, s);     // before c is written: c may be b
        launch_strided_round(c, cc, ac == cc ? nullptr : ac, now, false, s);
        if (shared_b) ring_tile_lt<A, true, true>(c, lt, cc, cc, b_hat, now * n, s);
        else ring_tile_lt<A, true, false>(c, lt, cc, cc, ws, now * n, s);
        launch_strided_round(c, cc, nullptr, now, true, s);
    }
}

static void refuse_large(const NttContext& c) {
    refuse_above_two_pass(c, "ring multiply on a context above n = 131072 is not supported (lsr_cyclic_ntt_context_create_large)");
}

// One call on the device (caller validated the arguments): workspace, ordering brackets, launches.
static void ring_mul_device(const NttContext& c, uint64_t* d_c, const uint64_t* d_a, const uint64_t* d_b, size_t batch, size_t b_rows, hipStream_t s) {
    refuse_large(c);
    const bool shared_b = b_rows == 1 && batch > 1;
    ring_call(c, c.ring_scratch, ring_scratch_words(c), c.logn > kTileLog || shared_b, s, [&] {
        for_flavour(c, [&](auto a) { ring_mul_enqueue<decltype(a)>(c, d_c, d_a, d_b, batch, shared_b, s); });
    });
}

// host buffers through bounded device chunks on the context's work stream
static void host_ring_mul(const NttContext& c, uint64_t* out, const uint64_t* a, const uint64_t* b, size_t batch, size_t b_rows) {
    refuse_large(c);
    const size_t n = c.degree;
    const bool shared_b = b_rows == 1 && batch > 1;
    // each operand within the bound; the product comes back in a's buffer
    host_staged(c, batch, staging_chunk(batch, n), {staged_items(a, out, n * 8), staged_items(b, nullptr, shared_b ? 0 : n * 8, n * 8)},
                [&](const StagedChunk& k, hipStream_t s) {
                    ring_mul_device(c, k.lane<uint64_t>(0), k.lane<const uint64_t>(0), k.lane<const uint64_t>(1), k.now, shared_b ? 1 : k.now, s);
                });
}

}  // namespace lsr

// ------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------
// Argument checks that need no device (and no dereference of ctx): -1 and a message, or 0 to go on.
static int ring_mul_check(const char* where, const NttContext* ctx, const void* c, const void* a, const void* b, size_t batch, size_t b_rows) {
    if (lsr::refuse_coeff_context(where, ctx)) return -1;
    if (!ctx || !c || !a || !b) return lsr::abi_refuse(where, "NULL context or buffer");
    if (b_rows != 1 && b_rows != batch)
        return lsr::abi_refuse(where, "b_rows must be 1 or batch (" + std::to_string(batch) + "), got " + std::to_string(b_rows));
    return 0;
}

extern "C" {

int lsr_ntt_ring_mul_batch(const NttContext* ctx, uint64_t* c, const uint64_t* a, const uint64_t* b, size_t batch, size_t b_rows) noexcept {
    if (ring_mul_check("lsr_ntt_ring_mul_batch", ctx, c, a, b, batch, b_rows) != 0) return -1;
    if (batch == 0) return 0;
    return lsr::abi_guarded("lsr_ntt_ring_mul_batch", [&] {
        lsr::require_device();
        lsr::host_ring_mul(*ctx, c, a, b, batch, b_rows);
    });
}

int lsr_ntt_ring_mul_batch_device(const NttContext* ctx, uint64_t* d_c, const uint64_t* d_a, const uint64_t* d_b, size_t batch, size_t b_rows,
                                  void* stream) noexcept {
    if (ring_mul_check("lsr_ntt_ring_mul_batch_device", ctx, d_c, d_a, d_b, batch, b_rows) != 0) return -1;
    if (batch == 0) return 0;
    return lsr::abi_guarded("lsr_ntt_ring_mul_batch_device", [&] {
        lsr::require_device();
        lsr::DeviceGuard guard(ctx->device);
        lsr::ring_mul_device(*ctx, d_c, d_a, d_b, batch, b_rows, static_cast<hipStream_t>(stream));
    });
}

}  // extern "C"
