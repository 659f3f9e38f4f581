// Gram matrices of bounded ring vectors in Z_q[X]/(X^n + 1) for ANY modulus q >= 2 (batch.h "Gram matrices under any modulus",
// DESIGN.md §5r): the cross, symmetric and symmetrised forms of lsr_ntt_ring_gram_batch / _sym2_batch on a ring handle (LsrRingMod,
// lsr_ring_mod.hip), at every n the handle admits.  The caller states l-infinity bounds on the centred operands; the device verifies
// them and reports per family (status), and the columns are taken in groups of what P = p1 p2 carries under those bounds
// (ring_mod_capacity_product).  Per chunk of families and group of columns:
//   1. ring_mod_gram_lift_kernel (ring_mod_checked_lift, lsr_ring_mod_call.hpp): every operand word read once, lifted for both primes into the two halves of the handle's Gram
//      workspace, bounds and range folded into the family's flag word (families in several groups: one check pass over the chunk's
//      whole families first, then lifts without the check);
//   2. launch_ntt forward in place on each half (a-hat and b-hat are contiguous: one launch per prime);
//   3. the register-blocked pointwise product of §5j into the workspace: ring_mod_gram_kernel for both primes in one launch, or — the
//      FP64 flavour's cross and symmetric forms, where the second prime costs a wave — ring_gram_kernel once per prime;
//   4. launch_ntt inverse in place on each half's outputs;
//   5. ring_mod_gram_reduce_kernel (ring_mod_gated_reduce): CRT and reduction mod q into g (accumulating from the second group on), zeros where the family's
//      flags are set, and status.
// The workspace is [2][ring_mod_gram_words()] words and the flag words: sized by the process-wide chunk size alone, allocated by the
// first eager call or by lsr_ring_mod_gram_prepare, never resized (ring_mod_call, lsr_ring_mod_call.hpp).
#include <algorithm>
#include <cstring>

#include "lambda_snark/batch.h"
#include "lsr_flavour.hpp"
#include "lsr_ring_gram.hpp"
#include "lsr_ring_mod_call.hpp"
#include "lsr_ring_mod_gram_kernels.hpp"
#include "lsr_runtime.hpp"

namespace lsr {

size_t ring_mod_gram_words() { return std::max<size_t>((size_t)1 << 23, ntt_chunk_bytes() / 32); }

static_assert(kGramMaxGridZ <= 2 * kRingModGramFlagWords, "one flag word per family of a chunk");
static_assert(2 * (LSR_RING_GRAM_MAX_VECTORS / 4) * (LSR_RING_GRAM_MAX_VECTORS / 4) <= 65535, "block pairs and primes share one grid axis");

struct ModGramCall {
    uint64_t* g;
    int32_t* status;
    const uint64_t *a, *b;     // b == nullptr: the symmetric form
    size_t batch, ra, rb, width;
    bool sym2;
    uint64_t bound_a, bound_b;   // as the caller gave them: 0 = none
};

// what a call takes of the workspace and of P
struct ModGramPlan {
    bool sym, one_set;           // one_set: b's transforms are a's (the symmetric form, or the cross form with b == a and rb == ra)
    size_t vectors, outs;        // operand vectors lifted per family; output polynomials per family
    uint64_t bound_a, bound_b;   // resolved: none -> floor(q / 2); the symmetric form holds a against bound_a twice
    uint64_t check_a;            // what a's words are held against: both bounds where b is a itself
    size_t capacity;             // columns per group that P carries (sym2: two products per column)
};

static ModGramPlan mod_gram_plan(const LsrRingMod& h, const ModGramCall& c) {
    ModGramPlan p{};
    const uint64_t half = h.q >> 1;
    p.sym = c.b == nullptr;
    p.one_set = p.sym || (c.b == c.a && c.rb == c.ra);
    p.vectors = p.one_set ? c.ra : c.ra + c.rb;
    p.outs = gram_outputs(c.ra, c.rb, p.sym || c.sym2);
    p.bound_a = c.bound_a ? c.bound_a : half;
    p.bound_b = p.sym ? p.bound_a : (c.bound_b ? c.bound_b : half);
    p.check_a = !p.sym && c.b == c.a ? std::min(p.bound_a, p.bound_b) : p.bound_a;
    p.capacity = ring_mod_capacity_product(h.q, h.n, p.bound_a, p.bound_b);
    if (c.sym2) p.capacity /= 2;
    return p;
}

// Both primes in one launch (the prime is the low bit of grid y), or one launch of the single-prime kernel per prime: decided per
// instantiation by the compiler's resource report (profiles/r34_ring_mod_gram_resource_usage.txt).  Carrying the second
// prime costs the FP64 flavour's cross and symmetric kernels a wave (70 VGPRs against 62: 7 waves per SIMD against 8).
template <class A, bool SYM2>
constexpr bool kModGramBothPrimes = !(std::is_same_v<A, ArithF64> && !SYM2);

template <class A>
static void gram_product(const LsrRingMod& h, uint64_t* ghat, const uint64_t* ahat, const uint64_t* bhat, const GramShape& shape, bool sym, bool sym2,
                         size_t families, hipStream_t s) {
    constexpr int E = kGramEdge<A>;
    const unsigned bi = (shape.ra + E - 1) / E, bl = (shape.rb + E - 1) / E, pairs = sym || sym2 ? bi * (bi + 1) / 2 : bi * bl;
    const size_t half = ring_mod_gram_words();
    const unsigned runs = static_cast<unsigned>((h.n + kGramThreads - 1) / kGramThreads);
    const GramModPrimes primes{{h.prime[0]->mod, h.prime[1]->mod}, half};
    if (sym2) {
        static_assert(kModGramBothPrimes<A, true>, "the symmetrised form runs both primes in one launch");
        hipLaunchKernelGGL((ring_mod_gram_kernel<A, E, true, true>), dim3(runs, 2 * pairs, static_cast<unsigned>(families)), dim3(kGramThreads), 0, s, ghat, ahat,
                           bhat, shape, primes);
        return;
    }
    for_bool(sym, [&](auto y) {
        constexpr bool kSym = decltype(y)::value;
        if constexpr (kModGramBothPrimes<A, false>) {
            hipLaunchKernelGGL((ring_mod_gram_kernel<A, E, kSym>), dim3(runs, 2 * pairs, static_cast<unsigned>(families)), dim3(kGramThreads), 0, s, ghat, ahat,
                               bhat, shape, primes);
        } else {
            for (int i = 0; i < 2; ++i)
                hipLaunchKernelGGL((ring_gram_kernel<A, E, kSym>), dim3(runs, pairs, static_cast<unsigned>(families)), dim3(kGramThreads), 0, s, ghat + i * half,
                                   ahat + i * half, bhat + i * half, shape, h.prime[i]->mod);
        }
    });
}

template <class A>
static void mod_gram_enqueue(const LsrRingMod& h, const ModGramCall& c, hipStream_t s) {
    const ModGramPlan p = mod_gram_plan(h, c);
    const size_t n = h.n, half = ring_mod_gram_words(), polys = half >> h.logn;
    const size_t a_fam = c.ra * c.width * n, b_fam = c.rb * c.width * n, g_fam = p.outs * n;
    uint64_t* const ws = h.gram_ws.ptr;
    uint32_t* const flags = ring_mod_gram_flags(h);
    const uint64_t* const b = p.one_set ? c.a : c.b;
    // Columns per group: what P carries and what the workspace holds of one family (>= 1: mod_gram_call).  Families per chunk: what
    // the workspace holds of such groups and their outputs, the chunks of a batch of equal size.  A family's flags must be complete
    // before its first reduce: with one group the check rides in the lift, else a pass without stores over the chunk's whole
    // families comes first.
    const size_t wmax = std::min({c.width, p.capacity, (polys - p.outs) / p.vectors});
    const size_t chunk_max = std::min(polys / (p.vectors * wmax + p.outs), kGramMaxGridZ);
    const size_t chunks = (c.batch + chunk_max - 1) / chunk_max, chunk = (c.batch + chunks - 1) / chunks;
    const bool one_group = wmax == c.width;
    const size_t vec_words = c.width * n;
    for (size_t j0 = 0; j0 < c.batch; j0 += chunk) {
        const size_t now = std::min(chunk, c.batch - j0);
        const uint64_t *aj = c.a + j0 * a_fam, *bj = b + j0 * b_fam;
        zero_words_async(reinterpret_cast<uint64_t*>(flags), (now + 1) / 2, s);
        if (!one_group) {
            ring_mod_checked_lift<true, false>(h, {ws, aj, c.ra, now, vec_words, vec_words, a_fam, 0, 0, half, p.check_a}, flags, s);
            if (!p.one_set) ring_mod_checked_lift<true, false>(h, {ws, bj, c.rb, now, vec_words, vec_words, b_fam, 0, 0, half, p.bound_b}, flags, s);
        }
        for (size_t c0 = 0; c0 < c.width; c0 += wmax) {
            const size_t wnow = std::min(wmax, c.width - c0), run = wnow * n;
            uint64_t* const bhat = p.one_set ? ws : ws + now * c.ra * run;
            uint64_t* const ghat = ws + now * p.vectors * run;
            const LiftLaunch la{ws, aj + c0 * n, c.ra, now, run, vec_words, a_fam, run, c.ra * run, half, p.check_a};
            const LiftLaunch lb{bhat, bj + c0 * n, c.rb, now, run, vec_words, b_fam, run, c.rb * run, half, p.bound_b};
            for_bool(one_group, [&](auto check) {
                ring_mod_checked_lift<decltype(check)::value, true>(h, la, flags, s);
                if (!p.one_set) ring_mod_checked_lift<decltype(check)::value, true>(h, lb, flags, s);
            });
            ring_mod_gram_transforms(h, ws, now * p.vectors * wnow, false, s);
            const GramShape shape{(uint32_t)h.logn, (uint32_t)c.ra, (uint32_t)c.rb, (uint32_t)wnow, kRingDotFirst | kRingDotLast,
                                  run, c.ra * run, run, c.rb * run, g_fam};
            gram_product<A>(h, ghat, ws, bhat, shape, p.sym, c.sym2, now, s);
            ring_mod_gram_transforms(h, ghat, now * p.outs, true, s);
            ring_mod_gated_reduce(h, c.g + j0 * g_fam, c.status + j0, ghat, ghat + half, flags, g_fam, now, c0 > 0, s);
        }
    }
}

// One call on the device (caller validated the arguments) in the handle's bracket (ring_mod_call), on its Gram workspace
static void mod_gram_device(const LsrRingMod& h, const ModGramCall& c, hipStream_t s) {
    ring_mod_call(h, s, true, [&] { for_ring_mod_flavour(h, [&](auto a) { mod_gram_enqueue<decltype(a)>(h, c, s); }); });
}

// host buffers through bounded device chunks of whole families on the first prime context's work stream; status comes back with g
static void host_mod_gram(const LsrRingMod& h, const ModGramCall& c) {
    const ModGramPlan p = mod_gram_plan(h, c);
    const NttContext& ctx = *h.prime[0];
    const size_t n = h.n, a_words = c.ra * c.width * n, b_words = p.one_set ? 0 : c.rb * c.width * n, g_words = p.outs * n;
    host_staged(ctx, c.batch, staging_chunk(c.batch, a_words + b_words + g_words),
                {staged_items(c.a, nullptr, a_words * 8), staged_items(c.b, nullptr, b_words * 8), staged_items(nullptr, c.g, g_words * 8),
                 staged_items(nullptr, c.status, sizeof(int32_t))},
                [&](const StagedChunk& k, hipStream_t s) {
                    ModGramCall d = c;
                    d.g = k.lane<uint64_t>(2);
                    d.status = k.lane<int32_t>(3);
                    d.a = k.lane<const uint64_t>(0);
                    d.b = p.sym ? nullptr : (p.one_set ? d.a : k.lane<const uint64_t>(1));
                    d.batch = k.now;
                    mod_gram_device(h, d, s);
                });
}

}  // namespace lsr

// ------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------
namespace {

// The refusals of batch.h in its order, all before any device work.  Up to the bounds they read nothing of the handle but q.
int mod_gram_call(const char* where, const LsrRingMod* h, const lsr::ModGramCall& c, bool device, void* stream) noexcept {
    if (!h || !c.g || !c.status || !c.a || (c.sym2 && !c.b)) return lsr::abi_refuse(where, "NULL handle, buffer or status");
    if (lsr::ring_gram_shape_check(where, c.b != nullptr, c.batch, c.ra, c.rb, c.width, c.sym2) != 0) return -1;
    if (lsr::ring_mod_bounds_check(where, h->q, "bound_a", c.bound_a, "bound_b", c.bound_b, c.b != nullptr) != 0) return -1;
    if (c.batch == 0) return 0;
    return lsr::abi_guarded(where, [&] {
        const lsr::ModGramPlan p = lsr::mod_gram_plan(*h, c);
        const size_t poly_bytes = (size_t)h->n * 8, listed = p.sym ? c.ra : c.ra + c.rb;
        // (at most 128 * 65536 and 4096 polynomials of at most 2^20 bytes: no overflow)
        if (listed * c.width * poly_bytes > LSR_RING_GRAM_MAX_FAMILY_BYTES || p.outs * poly_bytes > LSR_RING_GRAM_MAX_FAMILY_BYTES)
            throw std::runtime_error("one family takes " + std::to_string(listed * c.width * poly_bytes) + " bytes of operands and " +
                                     std::to_string(p.outs * poly_bytes) + " bytes of outputs: above LSR_RING_GRAM_MAX_FAMILY_BYTES (" +
                                     std::to_string((size_t)LSR_RING_GRAM_MAX_FAMILY_BYTES) + ")");
        const size_t polys = lsr::ring_mod_gram_words() >> h->logn;
        if (p.vectors + p.outs > polys)
            throw std::runtime_error("a family of " + std::to_string(p.vectors) + " vectors and " + std::to_string(p.outs) +
                                     " outputs needs a workspace of as many polynomials per prime even one column at a time; it holds " + std::to_string(polys) +
                                     " at this ring degree (LAMBDA_SNARK_NTT_CHUNK_MIB sets the workspace size)");
        if (c.sym2 && p.capacity == 0)
            throw std::runtime_error("the symmetrised form sums two products per column and q = " + std::to_string(h->q) + ", n = " + std::to_string(h->n) +
                                     " under these bounds carries one (lsr_ring_mod_capacity_product): take the cross form, lsr_ring_mod_gram_batch, "
                                     "and add its (i, l) and (l, i) entries mod q");
        size_t a_bytes = 0, b_bytes = 0, g_bytes = 0;
        if (__builtin_mul_overflow(c.batch * c.ra * c.width, poly_bytes, &a_bytes) || __builtin_mul_overflow(c.batch * c.rb * c.width, poly_bytes, &b_bytes) ||
            __builtin_mul_overflow(c.batch * p.outs, poly_bytes, &g_bytes))
            throw std::runtime_error("the sizes of a, b or g overflow size_t at this ring degree");
        lsr::require_outputs_apart({"g", c.g, g_bytes}, {"status", c.status, c.batch * sizeof(int32_t)}, {{"a", c.a, a_bytes}, {"b", c.b, b_bytes}});
        lsr::require_device();
        lsr::DeviceGuard guard(h->device);
        if (device) lsr::mod_gram_device(*h, c, static_cast<hipStream_t>(stream));
        else lsr::host_mod_gram(*h, c);
    });
}

}  // namespace

extern "C" {

size_t lsr_ring_mod_capacity_product(uint64_t q, uint32_t n, uint64_t bound_a, uint64_t bound_b) noexcept {
    try {
        return lsr::ring_mod_capacity_product(q, n, bound_a, bound_b);
    } catch (...) {
        return 0;
    }
}

int lsr_ring_mod_gram_prepare(const LsrRingMod* h) noexcept {
    const char* const where = "lsr_ring_mod_gram_prepare";
    if (!h) return lsr::abi_refuse(where, "NULL handle");
    return lsr::abi_guarded(where, [&] {
        lsr::require_device();
        lsr::DeviceGuard guard(h->device);
        std::lock_guard<std::mutex> lock(h->mutex);
        lsr::ring_mod_gram_workspace(*h);
    });
}

int lsr_ring_mod_gram_batch(const LsrRingMod* h, uint64_t* g, int32_t* status, const uint64_t* a, const uint64_t* b, size_t batch, size_t ra, size_t rb,
                            size_t width, uint64_t bound_a, uint64_t bound_b) noexcept {
    return mod_gram_call("lsr_ring_mod_gram_batch", h, {g, status, a, b, batch, ra, rb, width, false, bound_a, bound_b}, false, nullptr);
}
int lsr_ring_mod_gram_batch_device(const LsrRingMod* h, uint64_t* d_g, int32_t* d_status, const uint64_t* d_a, const uint64_t* d_b, size_t batch, size_t ra,
                                   size_t rb, size_t width, uint64_t bound_a, uint64_t bound_b, void* stream) noexcept {
    return mod_gram_call("lsr_ring_mod_gram_batch_device", h, {d_g, d_status, d_a, d_b, batch, ra, rb, width, false, bound_a, bound_b}, true, stream);
}
int lsr_ring_mod_gram_sym2_batch(const LsrRingMod* h, uint64_t* out, int32_t* status, const uint64_t* a, const uint64_t* b, size_t batch, size_t r,
                                 size_t width, uint64_t bound_a, uint64_t bound_b) noexcept {
    return mod_gram_call("lsr_ring_mod_gram_sym2_batch", h, {out, status, a, b, batch, r, r, width, true, bound_a, bound_b}, false, nullptr);
}
int lsr_ring_mod_gram_sym2_batch_device(const LsrRingMod* h, uint64_t* d_out, int32_t* d_status, const uint64_t* d_a, const uint64_t* d_b, size_t batch,
                                        size_t r, size_t width, uint64_t bound_a, uint64_t bound_b, void* stream) noexcept {
    return mod_gram_call("lsr_ring_mod_gram_sym2_batch_device", h, {d_out, d_status, d_a, d_b, batch, r, r, width, true, bound_a, bound_b}, true, stream);
}

}  // extern "C"
