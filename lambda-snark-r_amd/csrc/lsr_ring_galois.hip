// Galois automorphisms of ring elements (batch.h "Galois automorphisms"): out = sigma_g(x) as one streaming launch
// without a workspace, on every context and every n (it runs no transform), and the twisted inner product
// c_j = sum_{i < terms} sigma_g(a_{j,i}) b_{j,i} as lsr_ring_dot.hip's n <= 4096 schedule with the permutation and the sign applied
// where the tile kernel reads a, so that sigma_g(a) never exists in memory.  g is validated and inverted on the host; the kernels get
// h = g^-1 mod N and the mask N - 1 by value, which keeps the device forms enqueue-only and capturable.
#include <algorithm>

#include "lambda_snark/batch.h"
#include "lsr_flavour.hpp"
#include "lsr_ring_call.hpp"
#include "lsr_ring_galois_kernels.hpp"
#include "lsr_ring_workspace.hpp"
#include "lsr_runtime.hpp"

namespace lsr {

// N: the order of X in the context's ring
static uint64_t galois_order(const NttContext& c) { return c.cyclic ? (uint64_t)c.degree : 2 * (uint64_t)c.degree; }

// odd g < N = 2^k <= 2^23: Newton's iteration doubles the correct low bits of the inverse (g is its own inverse mod 8)
static GaloisParams galois_params(const NttContext& c, uint64_t g) {
    uint32_t h = (uint32_t)g;
    for (int i = 0; i < 4; ++i) h *= 2u - (uint32_t)g * h;
    const uint32_t mask = (uint32_t)(galois_order(c) - 1);
    return {h & mask, mask};
}

static void automorphism_device(const NttContext& c, uint64_t* d_out, const uint64_t* d_x, size_t count, uint64_t g, hipStream_t s) {
    const size_t total = count << c.logn;
    const dim3 grid(static_cast<unsigned>(std::min<size_t>((total + kTile - 1) / kTile, (size_t)1 << 20)));
    const GaloisParams gp = galois_params(c, g);
    if (c.logn <= kTileLog) hipLaunchKernelGGL(ring_automorphism_kernel<true>, grid, dim3(kThreads), 0, s, d_out, d_x, total, c.logn, gp, c.modulus);
    else hipLaunchKernelGGL(ring_automorphism_kernel<false>, grid, dim3(kThreads), 0, s, d_out, d_x, total, c.logn, gp, c.modulus);
    LSR_HIP(hipGetLastError());
}

struct DotGaloisOperands {
    uint64_t* c;
    const uint64_t *a, *b;
    size_t total;        // words of c
    uint32_t nterms;
    size_t a_os, b_os;   // words between consecutive outputs' term-i polynomials
    uint32_t flags;
    GaloisParams g;
};

template <class A, int LT, bool BHAT>
static void dot_galois_tile(const NttContext& c, const DotGaloisOperands& o, hipStream_t s) {
    const unsigned grid = static_cast<unsigned>((o.total + kTile - 1) / kTile);
    hipLaunchKernelGGL((ntt_tile_ring_dot_galois<A, LT, BHAT>), dim3(grid), dim3(kThreads), 0, s, o.c, o.a, o.b, o.total, o.nterms, o.a_os, o.b_os, o.flags,
                       o.g, c.mod, Flavour<A>::fwd(c), Flavour<A>::inv(c), Flavour<A>::consts(c));
}

template <class A, bool BHAT>
static void dot_galois_tile_lt(const NttContext& c, const DotGaloisOperands& o, hipStream_t s) {
    for_tile_log<1, 12>(c.logn, [&](auto t) { dot_galois_tile<A, decltype(t)::value, BHAT>(c, o, s); });
}

// n <= 4096; ring_dot_enqueue's schedule there (first / last: this call starts / finishes the sums)
template <class A>
static void ring_dot_galois_enqueue(const NttContext& c, uint64_t* d_c, const uint64_t* d_a, const uint64_t* d_b, size_t batch, size_t terms, bool shared_b,
                                    const GaloisParams& g, bool first, bool last, hipStream_t s) {
    const size_t n = c.degree, polys = ring_dot_chunk_polys(c);
    if (!shared_b) {
        dot_galois_tile_lt<A, false>(c, {d_c, d_a, d_b, batch * n, (uint32_t)terms, terms * n, terms * n, ring_dot_flags(first, last), g}, s);
        return;
    }
    uint64_t* const ws = c.ring_dot_scratch.ptr;
    for (size_t i0 = 0; i0 < terms; i0 += polys) {
        const size_t group = std::min(polys, terms - i0);
        launch_ntt(c, ws, group, false, s, nullptr, nullptr, d_b + i0 * n);
        dot_galois_tile_lt<A, true>(
            c, {d_c, d_a + i0 * n, ws, batch * n, (uint32_t)group, terms * n, 0, ring_dot_flags(first && i0 == 0, last && i0 + group == terms), g}, s);
    }
}

// One call on the device (caller validated the arguments): the ring inner product's workspace, ordering brackets and capture contract.
static void ring_dot_galois_device(const NttContext& c, uint64_t* d_c, const uint64_t* d_a, const uint64_t* d_b, size_t batch, size_t terms, size_t b_rows,
                                   uint64_t g, hipStream_t s, bool first = true, bool last = true) {
    const bool shared_b = b_rows == 1 && batch > 1;
    const GaloisParams gp = galois_params(c, g);
    ring_call(c, c.ring_dot_scratch, ring_dot_scratch_words(c), shared_b, s, [&] {
        for_flavour(c, [&](auto a) { ring_dot_galois_enqueue<decltype(a)>(c, d_c, d_a, d_b, batch, terms, shared_b, gp, first, last, s); });
    });
}

// (host buffers: host_staged and host_staged_dot, lsr_ring_call.hpp)

}  // namespace lsr

// ------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------
namespace {

// Steps 3 to 5 of batch.h's order, which read no context: -1 and a message, 1 for the empty call (a no-op), 0 to go on.  `polys`:
// the polynomials of each buffer (a product that overflowed arrives as SIZE_MAX).
int galois_check(const char* where, uint64_t g, bool empty, std::initializer_list<size_t> polys) {
    if ((g & 1) == 0) return lsr::abi_refuse(where, "g = " + std::to_string(g) + " is even: a Galois element is odd");
    if (empty) return 1;
    for (const size_t count : polys) {
        size_t bytes = 0;   // at the smallest ring (n = 2, 16 bytes a polynomial)
        if (count == SIZE_MAX || __builtin_mul_overflow(count, (size_t)16, &bytes)) return lsr::abi_refuse(where, "the sizes of the buffers overflow size_t");
    }
    return 0;
}

size_t mul_or_max(size_t x, size_t y) {
    size_t r = 0;
    return __builtin_mul_overflow(x, y, &r) ? SIZE_MAX : r;
}

// the checks of a non-empty call that read the context and both calls share: g < N, the byte sizes at this degree
void galois_validate(const NttContext& ctx, uint64_t g, std::initializer_list<size_t> polys) {
    const uint64_t order = lsr::galois_order(ctx);
    if (g >= order)
        throw std::runtime_error("g = " + std::to_string(g) + " is not below N = " + std::to_string(order) + " (N = " + (ctx.cyclic ? "n" : "2 n") +
                                 " on this context)");
    for (const size_t count : polys) {
        size_t bytes = 0;
        if (__builtin_mul_overflow(count, (size_t)ctx.degree * 8, &bytes)) throw std::runtime_error("the sizes of the buffers overflow size_t at this ring degree");
    }
}

int automorphism_call(const char* where, const NttContext* ctx, uint64_t* out, const uint64_t* x, size_t count, uint64_t g, bool device,
                      void* stream) noexcept {
    if (!ctx || !out || !x) return lsr::abi_refuse(where, "NULL context or buffer");
    const int rc = galois_check(where, g, count == 0, {count});
    if (rc != 0) return rc < 0 ? -1 : 0;
    return lsr::abi_guarded(where, [&] {
        galois_validate(*ctx, g, {count});
        const size_t n = ctx->degree;
        lsr::require_apart(out, count * n * 8, x, count * n * 8, "out overlaps x: there is no in-place form, the output must not share memory with the operand");
        lsr::require_device();
        if (device) {
            lsr::DeviceGuard guard(ctx->device);
            lsr::automorphism_device(*ctx, out, x, count, g, static_cast<hipStream_t>(stream));
        } else {
            lsr::host_staged(*ctx, out, x, count, n, n, [&](uint64_t* d_out, const uint64_t* d_in, size_t now, hipStream_t s) {
                lsr::automorphism_device(*ctx, d_out, d_in, now, g, s);
            });
        }
    });
}

int dot_galois_call(const char* where, const NttContext* ctx, uint64_t* c, const uint64_t* a, const uint64_t* b, size_t batch, size_t terms, size_t b_rows,
                    uint64_t g, bool device, void* stream) noexcept {
    if (lsr::refuse_coeff_context(where, ctx)) return -1;
    if (!ctx || !c || !a || !b) return lsr::abi_refuse(where, "NULL context or buffer");
    if (b_rows != 1 && b_rows != batch)
        return lsr::abi_refuse(where, "b_rows must be 1 or batch (" + std::to_string(batch) + "), got " + std::to_string(b_rows));
    if (terms == 0) return lsr::abi_refuse(where, "terms must be at least 1");
    const size_t a_polys = mul_or_max(batch, terms), b_polys = mul_or_max(b_rows, terms);
    const int rc = galois_check(where, g, batch == 0, {batch, a_polys, b_polys});
    if (rc != 0) return rc < 0 ? -1 : 0;
    return lsr::abi_guarded(where, [&] {
        galois_validate(*ctx, g, {batch, a_polys, b_polys});
        const size_t n = ctx->degree, poly_bytes = n * 8;
        if (ctx->logn > lsr::kTileLog)
            throw std::runtime_error("n = " + std::to_string(n) + " is above 4096, where the twisted inner product has no fused form: apply "
                                     "lsr_ntt_ring_automorphism_batch_device to a and pass the result to lsr_ntt_ring_dot_batch_device");
        if (terms > LSR_RING_DOT_MAX_TERMS)
            throw std::runtime_error("terms = " + std::to_string(terms) + " is above LSR_RING_DOT_MAX_TERMS (" + std::to_string(LSR_RING_DOT_MAX_TERMS) + ")");
        lsr::require_apart(c, batch * poly_bytes, a, a_polys * poly_bytes, "c overlaps a: the output must not share memory with an operand");
        lsr::require_apart(c, batch * poly_bytes, b, b_polys * poly_bytes, "c overlaps b: the output must not share memory with an operand");
        lsr::require_device();
        if (device) {
            lsr::DeviceGuard guard(ctx->device);
            lsr::ring_dot_galois_device(*ctx, c, a, b, batch, terms, b_rows, g, static_cast<hipStream_t>(stream));
        } else {
            lsr::host_staged_dot(*ctx, c, a, b, batch, terms, b_rows,
                                 [&](uint64_t* d_c, const uint64_t* d_a, const uint64_t* d_b, size_t now, size_t group, size_t rows, hipStream_t s, bool first,
                                     bool last) { lsr::ring_dot_galois_device(*ctx, d_c, d_a, d_b, now, group, rows, g, s, first, last); });
        }
    });
}

}  // namespace

extern "C" {

int lsr_ntt_ring_automorphism_batch(const NttContext* ctx, uint64_t* out, const uint64_t* x, size_t count, uint64_t g) noexcept {
    return automorphism_call("lsr_ntt_ring_automorphism_batch", ctx, out, x, count, g, false, nullptr);
}
int lsr_ntt_ring_automorphism_batch_device(const NttContext* ctx, uint64_t* d_out, const uint64_t* d_x, size_t count, uint64_t g, void* stream) noexcept {
    return automorphism_call("lsr_ntt_ring_automorphism_batch_device", ctx, d_out, d_x, count, g, true, stream);
}

int lsr_ntt_ring_dot_galois_batch(const NttContext* ctx, uint64_t* c, const uint64_t* a, const uint64_t* b, size_t batch, size_t terms, size_t b_rows,
                                  uint64_t g) noexcept {
    return dot_galois_call("lsr_ntt_ring_dot_galois_batch", ctx, c, a, b, batch, terms, b_rows, g, false, nullptr);
}
int lsr_ntt_ring_dot_galois_batch_device(const NttContext* ctx, uint64_t* d_c, const uint64_t* d_a, const uint64_t* d_b, size_t batch, size_t terms,
                                         size_t b_rows, uint64_t g, void* stream) noexcept {
    return dot_galois_call("lsr_ntt_ring_dot_galois_batch_device", ctx, d_c, d_a, d_b, batch, terms, b_rows, g, true, stream);
}

}  // extern "C"
