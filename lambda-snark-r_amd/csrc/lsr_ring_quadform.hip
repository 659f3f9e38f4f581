// Batched ring quadratic forms of a packed symmetric matrix:
//   out[j] = sum_i g[j][(i,i)] c_i c_i + offdiag * sum_{i < l} g[j][(i,l)] c_i c_l,
// g: [batch][r (r + 1) / 2][n] in the packed order of the symmetric ring Gram matrix, c: [c_rows][r][n] (c_rows == 1: one set of
// challenges for every family), out: [batch][n].  r + pairs forward transforms and ONE inverse per family instead of the 4 pairs
// forward and pairs + 1 inverse ones of a ring product per pair followed by a ring inner product, and no [pairs][n] temporary.  The
// Gram call's plan (lsr_ring_gram.hip), per chunk of families:
//   1. launch_ntt (forward, out of place) of c and of g into the ring inner product's workspace; g and c are never written (a shared
//      c is transformed once per call);
//   2. ring_quadform_kernel: the row-wise pointwise evaluation, the rows of the triangle split over grid.y into slices balanced by
//      pairs; with more than one slice ring_quadform_reduce_kernel adds the slices' partials (workspace) in slice order;
//   3. launch_ntt (inverse) in place on the outputs.
// A family whose r + pairs (+ slices) polynomials do not fit the workspace is taken in groups of consecutive packed pairs with c-hat
// resident, the running sum waiting in out as canonical evaluation-domain words between groups (kRingDotFirst), as the Gram call's
// column groups do.  (Groups are runs of the packed order, not whole rows: the kernel takes a row in pieces anyway, since slices are
// balanced by pairs, and a workspace of r + 2 polynomials is enough.)
// One path for every n <= 131072, every flavour, cyclic and negacyclic contexts.  The workspace is ring_dot_scratch
// (lsr_ring_workspace.hpp), under the same mutex and event as the ring inner product.
#include <algorithm>
#include <cstring>

#include "lambda_snark/batch.h"
#include "lsr_flavour.hpp"
#include "lsr_ring_call.hpp"
#include "lsr_ring_quadform_kernels.hpp"
#include "lsr_ring_workspace.hpp"
#include "lsr_runtime.hpp"

namespace lsr {

constexpr size_t kQuadMaxFamilies = 65535;     // one grid axis
constexpr size_t kQuadTargetGroups = 1024;     // workgroups a launch should reach before the triangle is left in one slice (4 per CU)
constexpr size_t kQuadMinSlicePairs = 4;       // a slice pays 2 products and a c-hat_i load per row it touches
constexpr size_t kQuadMaxSlices = 64;

// polynomials the workspace holds: both halves of the n > 4096 layout
static size_t quad_workspace_polys(const NttContext& c) { return ring_dot_scratch_words(c) >> c.logn; }

static unsigned quad_threads(const NttContext& c) { return std::min<unsigned>(kQuadThreads, std::max<unsigned>(64, c.degree)); }

// slices of a launch over `count` pairs of `families` families, at most `cap`
static size_t quad_slices(const NttContext& c, size_t families, size_t count, size_t cap) {
    const size_t threads = quad_threads(c), groups = (c.degree + threads - 1) / threads * families;
    const size_t want = (kQuadTargetGroups + groups - 1) / groups, most = (count + kQuadMinSlicePairs - 1) / kQuadMinSlicePairs;
    return std::max<size_t>(1, std::min({want, most, cap, kQuadMaxSlices}));
}

// One launch over the packed pairs [p0, p1) of `families` families (g-hat holds them from p0 on), and the reduction of its slices.
template <class A>
static void quad_launch(const NttContext& c, uint64_t* out, uint64_t* part, const uint64_t* ghat, const uint64_t* chat, size_t r, size_t p0,
                        size_t p1, size_t slices, size_t c_fam, size_t g_fam, uint64_t offdiag, bool first, size_t families, hipStream_t s) {
    const unsigned threads = quad_threads(c), runs = (c.degree + threads - 1) / threads;
    const QuadShape shape{(uint32_t)c.logn, (uint32_t)r, first ? kRingDotFirst : 0u, (uint32_t)p0, (uint32_t)p1, (uint32_t)slices, c_fam, g_fam, offdiag};
    hipLaunchKernelGGL((ring_quadform_kernel<A>), dim3(runs, (unsigned)slices, (unsigned)families), dim3(threads), 0, s, out, part, ghat, chat, shape,
                       c.mod);
    if (slices > 1)
        hipLaunchKernelGGL((ring_quadform_reduce_kernel<std::is_same_v<A, ArithGold>>), dim3(runs, (unsigned)families), dim3(threads), 0, s, out, part,
                           (uint32_t)c.logn, (uint32_t)slices, shape.flags, c.modulus);
}

template <class A>
static void ring_quadform_enqueue(const NttContext& c, uint64_t* d_out, const uint64_t* d_g, const uint64_t* d_c, size_t batch, size_t r,
                                  size_t c_rows, uint64_t offdiag, hipStream_t s) {
    const size_t n = c.degree, polys = quad_workspace_polys(c), pairs = r * (r + 1) / 2;
    const bool shared = c_rows == 1;
    uint64_t* const ws = c.ring_dot_scratch.ptr;
    // chunks of whole families: [c-hat: r per family, or r once][g-hat: pairs per family][partials: slices per family]
    const size_t rest = polys - (shared ? r : 0);          // polys >= r + 2: ring_quadform_validate
    size_t slices = quad_slices(c, std::min(batch, kQuadMaxFamilies), pairs, pairs);
    auto per_family = [&](size_t sl) { return (shared ? 0 : r) + pairs + (sl > 1 ? sl : 0); };
    if (per_family(slices) > rest) slices = 1;
    if (per_family(slices) <= rest) {
        const size_t chunk = std::min({rest / per_family(slices), kQuadMaxFamilies, batch});
        uint64_t* const ghat = ws + (shared ? 1 : chunk) * r * n;
        uint64_t* const part = ghat + chunk * pairs * n;
        if (shared) launch_ntt(c, ws, r, false, s, nullptr, nullptr, d_c);
        for (size_t j0 = 0; j0 < batch; j0 += chunk) {
            const size_t now = std::min(chunk, batch - j0);
            if (!shared) launch_ntt(c, ws, now * r, false, s, nullptr, nullptr, d_c + j0 * r * n);
            launch_ntt(c, ghat, now * pairs, false, s, nullptr, nullptr, d_g + j0 * pairs * n);
            quad_launch<A>(c, d_out + j0 * n, part, ghat, ws, r, 0, pairs, slices, shared ? 0 : r * n, pairs * n, offdiag, true, now, s);
            launch_ntt(c, d_out + j0 * n, now, true, s);
        }
        return;
    }
    // one family at a time, c-hat resident, g in groups of consecutive packed pairs: [c-hat: r][g-hat: group][partials: slices]
    const size_t room = polys - r;                         // >= 2
    slices = quad_slices(c, 1, std::min(pairs, room - 1), room / 2);
    const size_t group = room - slices;
    uint64_t* const ghat = ws + r * n;
    uint64_t* const part = ghat + group * n;
    for (size_t j = 0; j < batch; ++j) {
        if (!shared || j == 0) launch_ntt(c, ws, r, false, s, nullptr, nullptr, d_c + (shared ? 0 : j * r * n));
        for (size_t p0 = 0; p0 < pairs; p0 += group) {
            const size_t now = std::min(group, pairs - p0);
            launch_ntt(c, ghat, now, false, s, nullptr, nullptr, d_g + (j * pairs + p0) * n);
            quad_launch<A>(c, d_out + j * n, part, ghat, ws, r, p0, p0 + now, std::min(slices, now), 0, 0, offdiag, p0 == 0, 1, s);
        }
    }
    launch_ntt(c, d_out, batch, true, s);
}

// One call on the device (caller validated the arguments): workspace, ordering brackets, launches.
static void ring_quadform_device(const NttContext& c, uint64_t* d_out, const uint64_t* d_g, const uint64_t* d_c, size_t batch, size_t r,
                                 size_t c_rows, uint64_t offdiag, hipStream_t s) {
    ring_call(c, c.ring_dot_scratch, ring_dot_scratch_words(c), true, s, [&] {
        for_flavour(c, [&](auto a) { ring_quadform_enqueue<decltype(a)>(c, d_out, d_g, d_c, batch, r, c_rows, offdiag, s); });
    });
}

// host buffers through bounded device chunks of whole families on the context's work stream (the two-operand loop of host_ring_gram;
// a shared c goes up once)
static void host_ring_quadform(const NttContext& c, uint64_t* out, const uint64_t* g, const uint64_t* cc, size_t batch, size_t r, size_t c_rows,
                               uint64_t offdiag) {
    const size_t n = c.degree;
    const bool shared = c_rows == 1;
    const size_t g_words = r * (r + 1) / 2 * n, c_words = r * n;
    host_staged(c, batch, staging_chunk(batch, g_words + c_words + n),
                {staged_items(g, nullptr, g_words * 8), staged_items(cc, nullptr, shared ? 0 : c_words * 8, c_words * 8), staged_items(nullptr, out, n * 8)},
                [&](const StagedChunk& k, hipStream_t s) {
                    ring_quadform_device(c, k.lane<uint64_t>(2), k.lane<const uint64_t>(0), k.lane<const uint64_t>(1), k.now, r, shared ? 1 : k.now, offdiag, s);
                });
}

}  // namespace lsr

// ------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------
namespace {

// Argument checks that read no context (and never dereference ctx), in the documented order: -1 and a message, 1 for the empty call
// (a no-op), 0 to go on.
int ring_quadform_check(const char* where, const NttContext* ctx, const void* out, const void* g, const void* c, size_t batch, size_t r,
                        size_t c_rows) {
    if (lsr::refuse_coeff_context(where, ctx)) return -1;
    if (!ctx || !out || !g || !c) return lsr::abi_refuse(where, "NULL context or buffer");
    if (r == 0) return lsr::abi_refuse(where, "r must be at least 1");
    if (c_rows != 1 && c_rows != batch)
        return lsr::abi_refuse(where, "c_rows must be 1 (one set of challenges for every family) or batch, got c_rows = " + std::to_string(c_rows) +
                                          ", batch = " + std::to_string(batch));
    if (r > LSR_RING_GRAM_MAX_VECTORS)
        return lsr::abi_refuse(where, "r = " + std::to_string(r) + " is above LSR_RING_GRAM_MAX_VECTORS (" + std::to_string(LSR_RING_GRAM_MAX_VECTORS) + ")");
    // in polynomials and then in bytes at the smallest ring (n = 2, 16 bytes a polynomial)
    size_t g_polys = 0, c_polys = 0, bytes = 0;
    const bool overflow = __builtin_mul_overflow(batch, r * (r + 1) / 2, &g_polys) || __builtin_mul_overflow(c_rows, r, &c_polys) ||
                          __builtin_mul_overflow(g_polys, (size_t)16, &bytes) || __builtin_mul_overflow(c_polys, (size_t)16, &bytes) ||
                          __builtin_mul_overflow(batch, (size_t)16, &bytes);
    if (overflow) return lsr::abi_refuse(where, "the sizes of g, c or out overflow size_t (batch, r, c_rows)");
    return batch == 0 ? 1 : 0;
}

// The checks of a non-empty call that read the context, still before any device work.
void ring_quadform_validate(const NttContext& ctx, const uint64_t* out, const uint64_t* g, const uint64_t* c, size_t batch, size_t r, size_t c_rows,
                            uint64_t offdiag) {
    lsr::refuse_above_two_pass(ctx, "ring quadratic form on a context above n = 131072 is not supported (lsr_cyclic_ntt_context_create_large)");
    if (offdiag >= ctx.modulus)
        throw std::runtime_error("offdiag = " + std::to_string(offdiag) + " is not a canonical word: the modulus is " + std::to_string(ctx.modulus));
    const size_t poly_bytes = (size_t)ctx.degree * 8, pairs = r * (r + 1) / 2;
    // (at most 2080 polynomials of at most 2^20 bytes: no overflow)
    if (pairs * poly_bytes > LSR_RING_GRAM_MAX_FAMILY_BYTES)
        throw std::runtime_error("one family's g takes " + std::to_string(pairs * poly_bytes) + " bytes: above LSR_RING_GRAM_MAX_FAMILY_BYTES (" +
                                 std::to_string((size_t)LSR_RING_GRAM_MAX_FAMILY_BYTES) + ")");
    const size_t polys = lsr::quad_workspace_polys(ctx);
    if (r + 2 > polys)
        throw std::runtime_error("r = " + std::to_string(r) + " challenges need a workspace of r + 2 polynomials (the transformed c, one of g, one partial sum); it holds " +
                                 std::to_string(polys) + " at this ring degree (LAMBDA_SNARK_NTT_CHUNK_MIB sets the workspace size)");
    size_t out_bytes = 0, g_bytes = 0, c_bytes = 0;
    if (__builtin_mul_overflow(batch, poly_bytes, &out_bytes) || __builtin_mul_overflow(batch * pairs, poly_bytes, &g_bytes) ||
        __builtin_mul_overflow(c_rows * r, poly_bytes, &c_bytes))
        throw std::runtime_error("the sizes of g, c or out overflow size_t at this ring degree");
    lsr::require_apart(out, out_bytes, g, g_bytes, "out overlaps g: the output must not share memory with an operand");
    lsr::require_apart(out, out_bytes, c, c_bytes, "out overlaps c: the output must not share memory with an operand");
    lsr::require_device();
}

}  // namespace

extern "C" {

int lsr_ntt_ring_quadform_batch(const NttContext* ctx, uint64_t* out, const uint64_t* g, const uint64_t* c, size_t batch, size_t r, size_t c_rows,
                                uint64_t offdiag) noexcept {
    const int rc = ring_quadform_check("lsr_ntt_ring_quadform_batch", ctx, out, g, c, batch, r, c_rows);
    if (rc != 0) return rc < 0 ? -1 : 0;
    return lsr::abi_guarded("lsr_ntt_ring_quadform_batch", [&] {
        ring_quadform_validate(*ctx, out, g, c, batch, r, c_rows, offdiag);
        lsr::host_ring_quadform(*ctx, out, g, c, batch, r, c_rows, offdiag);
    });
}

int lsr_ntt_ring_quadform_batch_device(const NttContext* ctx, uint64_t* d_out, const uint64_t* d_g, const uint64_t* d_c, size_t batch, size_t r,
                                       size_t c_rows, uint64_t offdiag, void* stream) noexcept {
    const int rc = ring_quadform_check("lsr_ntt_ring_quadform_batch_device", ctx, d_out, d_g, d_c, batch, r, c_rows);
    if (rc != 0) return rc < 0 ? -1 : 0;
    return lsr::abi_guarded("lsr_ntt_ring_quadform_batch_device", [&] {
        ring_quadform_validate(*ctx, d_out, d_g, d_c, batch, r, c_rows, offdiag);
        lsr::DeviceGuard guard(ctx->device);
        lsr::ring_quadform_device(*ctx, d_out, d_g, d_c, batch, r, c_rows, offdiag, static_cast<hipStream_t>(stream));
    });
}

}  // extern "C"
