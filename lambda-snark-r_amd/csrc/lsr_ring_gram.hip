// Batched ring Gram matrices G = A B^T:
//   g[j][i][l] = sum_{c < width} a[j][i][c] * b[j][l][c],   a: [batch][ra][width][n], b: [batch][rb][width][n], g: [batch][ra][rb][n],
// or, b == NULL, the packed upper triangle i <= l of a family with itself ([batch][r (r + 1) / 2][n]).  Every operand polynomial is
// transformed ONCE: (ra + rb) width forward transforms and one inverse per output instead of the 2 width + 1 transforms per output of
// a ring inner product on gathered operands, and no gathered copy.  Per chunk of families (or, for a family that does not fit the
// workspace, per group of columns of one family):
//   1. launch_ntt (forward, out of place) of the operands into the ring inner product's workspace; the caller's a and b are never written;
//   2. ring_gram_kernel: the register-blocked pointwise product, canonical evaluation-domain words into g (a later column group
//      loads them and adds: kRingDotFirst / kRingDotLast);
//   3. after the last group launch_ntt (inverse) in place on the outputs in g.
// The symmetrised form (lsr_ntt_ring_gram_sym2_batch): h[j][(i, l)] = <a_i, b_l> + <a_l, b_i> for i < l and <a_i, b_i> on
// the diagonal, packed as the symmetric form's g — the same plan with ra = rb = r and the SYM2 mode of the kernel.
// One path for every n <= 131072, every flavour, cyclic and negacyclic contexts.  The workspace is ring_dot_scratch
// (lsr_ring_workspace.hpp), under the same mutex and event as the ring inner product.
#include <algorithm>
#include <cstring>

#include "lambda_snark/batch.h"
#include "lsr_flavour.hpp"
#include "lsr_ring_call.hpp"
#include "lsr_ring_gram.hpp"
#include "lsr_ring_gram_kernels.hpp"
#include "lsr_ring_workspace.hpp"
#include "lsr_runtime.hpp"

namespace lsr {

// polynomials the workspace holds: both halves of the n > 4096 layout
static size_t gram_workspace_polys(const NttContext& c) { return ring_dot_scratch_words(c) >> c.logn; }

// sym: the packed upper triangle (b-hat == a-hat); sym2: the packed symmetrised form of two families
template <class A>
static void gram_launch(const NttContext& c, uint64_t* g, const uint64_t* ahat, const uint64_t* bhat, const GramShape& shape, bool sym, bool sym2,
                        size_t families, hipStream_t s) {
    constexpr int E = kGramEdge<A>;
    const unsigned bi = (shape.ra + E - 1) / E, bl = (shape.rb + E - 1) / E;
    const dim3 grid(static_cast<unsigned>((c.degree + kGramThreads - 1) / kGramThreads), sym || sym2 ? bi * (bi + 1) / 2 : bi * bl,
                    static_cast<unsigned>(families));
    if (sym2) {
        hipLaunchKernelGGL((ring_gram_kernel<A, E, true, true>), grid, dim3(kGramThreads), 0, s, g, ahat, bhat, shape, c.mod);
        return;
    }
    for_bool(sym, [&](auto y) {
        hipLaunchKernelGGL((ring_gram_kernel<A, E, decltype(y)::value>), grid, dim3(kGramThreads), 0, s, g, ahat, bhat, shape, c.mod);
    });
}

// b == nullptr: the symmetric form.  b == a with rb == ra: the cross form on ONE set of transforms.  sym2 (b != nullptr, rb == ra):
// the symmetrised packed form.
template <class A>
static void ring_gram_enqueue(const NttContext& c, uint64_t* d_g, const uint64_t* d_a, const uint64_t* d_b, size_t batch, size_t ra, size_t rb,
                              size_t width, bool sym2, hipStream_t s) {
    const size_t n = c.degree, polys = gram_workspace_polys(c);
    const bool sym = d_b == nullptr, one_set = sym || (d_b == d_a && rb == ra);
    const size_t vectors = sym ? ra : ra + rb, outs = gram_outputs(ra, rb, sym || sym2);
    const size_t a_fam = ra * width * n, b_fam = rb * width * n, g_fam = outs * n;
    uint64_t* const ws = c.ring_dot_scratch.ptr;
    if (one_set) d_b = d_a;
    if (vectors * width <= polys) {     // chunks of whole families: a chunk's operands are contiguous in a and in b
        const size_t chunk = std::min(polys / (vectors * width), kGramMaxGridZ);
        for (size_t j0 = 0; j0 < batch; j0 += chunk) {
            const size_t now = std::min(chunk, batch - j0);
            uint64_t* const bhat = one_set ? ws : ws + now * a_fam;
            launch_ntt(c, ws, now * ra * width, false, s, nullptr, nullptr, d_a + j0 * a_fam);
            if (!one_set) launch_ntt(c, bhat, now * rb * width, false, s, nullptr, nullptr, d_b + j0 * b_fam);
            const GramShape shape{(uint32_t)c.logn, (uint32_t)ra, (uint32_t)rb, (uint32_t)width, ring_dot_flags(true, true),
                                  width * n, a_fam, width * n, b_fam, g_fam};
            gram_launch<A>(c, d_g + j0 * g_fam, ws, bhat, shape, sym, sym2, now, s);
            launch_ntt(c, d_g + j0 * g_fam, now * outs, true, s);
        }
        return;
    }
    // one family at a time in groups of columns: the columns of a group are contiguous within a vector, not across vectors — one
    // forward launch per vector
    const size_t wmax = polys / vectors;     // >= 1: ring_gram_validate
    for (size_t j = 0; j < batch; ++j) {
        for (size_t c0 = 0; c0 < width; c0 += wmax) {
            const size_t wnow = std::min(wmax, width - c0);
            uint64_t* const bhat = one_set ? ws : ws + ra * wnow * n;
            for (size_t i = 0; i < ra; ++i) launch_ntt(c, ws + i * wnow * n, wnow, false, s, nullptr, nullptr, d_a + j * a_fam + (i * width + c0) * n);
            if (!one_set)
                for (size_t l = 0; l < rb; ++l)
                    launch_ntt(c, bhat + l * wnow * n, wnow, false, s, nullptr, nullptr, d_b + j * b_fam + (l * width + c0) * n);
            const GramShape shape{(uint32_t)c.logn, (uint32_t)ra, (uint32_t)rb, (uint32_t)wnow, ring_dot_flags(c0 == 0, c0 + wnow == width),
                                  wnow * n, 0, wnow * n, 0, g_fam};
            gram_launch<A>(c, d_g + j * g_fam, ws, bhat, shape, sym, sym2, 1, s);
        }
        launch_ntt(c, d_g + j * g_fam, outs, true, s);
    }
}

// One call on the device (caller validated the arguments): workspace, ordering brackets, launches.
static void ring_gram_device(const NttContext& c, uint64_t* d_g, const uint64_t* d_a, const uint64_t* d_b, size_t batch, size_t ra, size_t rb,
                             size_t width, bool sym2, hipStream_t s) {
    ring_call(c, c.ring_dot_scratch, ring_dot_scratch_words(c), true, s, [&] {
        for_flavour(c, [&](auto a) { ring_gram_enqueue<decltype(a)>(c, d_g, d_a, d_b, batch, ra, rb, width, sym2, s); });
    });
}

// host buffers through bounded device chunks of whole families on the context's work stream; the b lane is absent in the symmetric
// form and when b == a with rb == ra, where a goes up once and serves as both
static void host_ring_gram(const NttContext& c, uint64_t* g, const uint64_t* a, const uint64_t* b, size_t batch, size_t ra, size_t rb, size_t width,
                           bool sym2) {
    const size_t n = c.degree;
    const bool sym = b == nullptr, one_set = sym || (b == a && rb == ra);
    const size_t a_words = ra * width * n, b_words = one_set ? 0 : rb * width * n, g_words = gram_outputs(ra, rb, sym || sym2) * n;
    host_staged(c, batch, staging_chunk(batch, a_words + b_words + g_words),
                {staged_items(a, nullptr, a_words * 8), staged_items(b, nullptr, b_words * 8), staged_items(nullptr, g, g_words * 8)},
                [&](const StagedChunk& k, hipStream_t s) {
                    const uint64_t* const d_a = k.lane<const uint64_t>(0);
                    ring_gram_device(c, k.lane<uint64_t>(2), d_a, sym ? nullptr : (one_set ? d_a : k.lane<const uint64_t>(1)), k.now, ra, rb, width, sym2, s);
                });
}

}  // namespace lsr

// ------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------
namespace {

// Argument checks that read no context (and never dereference ctx), in the documented order: -1 and a message, 1 for the empty call
// (a no-op), 0 to go on.  sym2: the symmetrised form, whose b must not be NULL.
int ring_gram_check(const char* where, const NttContext* ctx, const void* g, const void* a, const void* b, size_t batch, size_t ra, size_t rb,
                    size_t width, bool sym2 = false) {
    if (lsr::refuse_coeff_context(where, ctx)) return -1;
    if (!ctx || !g || !a || (sym2 && !b)) return lsr::abi_refuse(where, "NULL context or buffer");
    if (lsr::ring_gram_shape_check(where, b != nullptr, batch, ra, rb, width, sym2) != 0) return -1;
    return batch == 0 ? 1 : 0;
}

// The checks of a non-empty call that read the context, still before any device work.
void ring_gram_validate(const NttContext& ctx, const uint64_t* g, const uint64_t* a, const uint64_t* b, size_t batch, size_t ra, size_t rb,
                        size_t width, bool sym2 = false) {
    lsr::refuse_above_two_pass(ctx, "ring Gram matrix on a context above n = 131072 is not supported (lsr_cyclic_ntt_context_create_large)");
    const bool sym = b == nullptr;
    const size_t poly_bytes = (size_t)ctx.degree * 8, vectors = sym ? ra : ra + rb, outs = lsr::gram_outputs(ra, rb, sym || sym2);
    // (at most 128 * 65536 and 4096 polynomials of at most 2^20 bytes: no overflow)
    if (vectors * width * poly_bytes > LSR_RING_GRAM_MAX_FAMILY_BYTES || outs * poly_bytes > LSR_RING_GRAM_MAX_FAMILY_BYTES)
        throw std::runtime_error("one family takes " + std::to_string(vectors * width * poly_bytes) + " bytes of operands and " +
                                 std::to_string(outs * poly_bytes) + " bytes of outputs: above LSR_RING_GRAM_MAX_FAMILY_BYTES (" +
                                 std::to_string((size_t)LSR_RING_GRAM_MAX_FAMILY_BYTES) + ")");
    const size_t polys = lsr::gram_workspace_polys(ctx);
    if (vectors > polys)
        throw std::runtime_error("a family of " + std::to_string(vectors) + " vectors needs a workspace of as many polynomials; it holds " +
                                 std::to_string(polys) + " at this ring degree (LAMBDA_SNARK_NTT_CHUNK_MIB sets the workspace size)");
    size_t a_bytes = 0, b_bytes = 0, g_bytes = 0;
    if (__builtin_mul_overflow(batch * ra * width, poly_bytes, &a_bytes) || __builtin_mul_overflow(batch * rb * width, poly_bytes, &b_bytes) ||
        __builtin_mul_overflow(batch * outs, poly_bytes, &g_bytes))
        throw std::runtime_error("the sizes of a, b or g overflow size_t at this ring degree");
    lsr::require_apart(g, g_bytes, a, a_bytes, "g overlaps a: the output must not share memory with an operand");
    if (b) lsr::require_apart(g, g_bytes, b, b_bytes, "g overlaps b: the output must not share memory with an operand");
    lsr::require_device();
}

}  // namespace

extern "C" {

int lsr_ntt_ring_gram_batch(const NttContext* ctx, uint64_t* g, const uint64_t* a, const uint64_t* b, size_t batch, size_t ra, size_t rb,
                            size_t width) noexcept {
    const int rc = ring_gram_check("lsr_ntt_ring_gram_batch", ctx, g, a, b, batch, ra, rb, width);
    if (rc != 0) return rc < 0 ? -1 : 0;
    return lsr::abi_guarded("lsr_ntt_ring_gram_batch", [&] {
        ring_gram_validate(*ctx, g, a, b, batch, ra, rb, width);
        lsr::host_ring_gram(*ctx, g, a, b, batch, ra, rb, width, false);
    });
}

int lsr_ntt_ring_gram_batch_device(const NttContext* ctx, uint64_t* d_g, const uint64_t* d_a, const uint64_t* d_b, size_t batch, size_t ra,
                                   size_t rb, size_t width, void* stream) noexcept {
    const int rc = ring_gram_check("lsr_ntt_ring_gram_batch_device", ctx, d_g, d_a, d_b, batch, ra, rb, width);
    if (rc != 0) return rc < 0 ? -1 : 0;
    return lsr::abi_guarded("lsr_ntt_ring_gram_batch_device", [&] {
        ring_gram_validate(*ctx, d_g, d_a, d_b, batch, ra, rb, width);
        lsr::DeviceGuard guard(ctx->device);
        lsr::ring_gram_device(*ctx, d_g, d_a, d_b, batch, ra, rb, width, false, static_cast<hipStream_t>(stream));
    });
}

int lsr_ntt_ring_gram_sym2_batch(const NttContext* ctx, uint64_t* h, const uint64_t* a, const uint64_t* b, size_t batch, size_t r,
                                 size_t width) noexcept {
    const int rc = ring_gram_check("lsr_ntt_ring_gram_sym2_batch", ctx, h, a, b, batch, r, r, width, true);
    if (rc != 0) return rc < 0 ? -1 : 0;
    return lsr::abi_guarded("lsr_ntt_ring_gram_sym2_batch", [&] {
        ring_gram_validate(*ctx, h, a, b, batch, r, r, width, true);
        lsr::host_ring_gram(*ctx, h, a, b, batch, r, r, width, true);
    });
}

int lsr_ntt_ring_gram_sym2_batch_device(const NttContext* ctx, uint64_t* d_h, const uint64_t* d_a, const uint64_t* d_b, size_t batch, size_t r,
                                        size_t width, void* stream) noexcept {
    const int rc = ring_gram_check("lsr_ntt_ring_gram_sym2_batch_device", ctx, d_h, d_a, d_b, batch, r, r, width, true);
    if (rc != 0) return rc < 0 ? -1 : 0;
    return lsr::abi_guarded("lsr_ntt_ring_gram_sym2_batch_device", [&] {
        ring_gram_validate(*ctx, d_h, d_a, d_b, batch, r, r, width, true);
        lsr::DeviceGuard guard(ctx->device);
        lsr::ring_gram_device(*ctx, d_h, d_a, d_b, batch, r, r, width, true, static_cast<hipStream_t>(stream));
    });
}

size_t lsr_ntt_ring_gram_block(const NttContext* ctx) noexcept {
    if (!ctx || lsr::refuse_coeff_context("lsr_ntt_ring_gram_block", ctx)) return 0;
    return lsr::for_flavour(*ctx, [](auto a) -> size_t { return lsr::kGramEdge<decltype(a)>; });
}

}  // extern "C"
