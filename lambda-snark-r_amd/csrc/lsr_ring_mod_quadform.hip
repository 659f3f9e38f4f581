// Ring quadratic forms of a packed Gram triangle in Z_q[X]/(X^n + 1) for ANY modulus q >= 2 (batch.h "quadratic forms under any
// modulus"): lsr_ntt_ring_quadform_batch on a ring handle (LsrRingMod, lsr_ring_mod.hip), at every n the handle admits,
//   out[j] = sum_i g[j][(i,i)] c_i c_i + offdiag * sum_{i < l} g[j][(i,l)] c_i c_l,
// with the bounds and the status of the Gram calls (lsr_ring_mod_gram.hip).  The form is CUBIC in its operands: a coefficient of one
// lifted triple product reaches n^2 bound_g bound_c^2, so the packed pairs are taken in groups of what P = p1 p2 carries of such
// products (ring_mod_capacity_quadform), an off-diagonal pair counting max(1, |w|) times for the centred offdiag w.  The caller states
// l-infinity bounds on the centred words of g and of c; the device verifies them and reports per family (status).  Per chunk of
// families and group of pairs, on the handle's Gram workspace:
//   1. the flag words cleared (a shared c: set to what its check found);
//   2. ring_mod_gram_lift_kernel: the group's g and (first group) the chunk's c read once, lifted for both primes, bounds and range
//      folded into the family's flag word — a shared c is lifted, checked and transformed once per call (a family in several groups:
//      one check pass without stores over the chunk's whole g first, so that its flags are complete before its first reduce);
//   3. launch_ntt forward in place on each half;
//   4. ring_mod_quadform_kernel: the row-wise evaluation for both primes in one launch, its slices' partials added by
//      ring_mod_quadform_sum_kernel;
//   5. launch_ntt inverse in place on each half's sums;
//   6. ring_mod_gram_reduce_kernel: CRT and reduction mod q into out (accumulating from the second group on), zeros where the family's
//      flags are set, and status.
// The lift and the reduce are launched by lsr_ring_mod_call.hpp, which also holds the bracket of a call and the Gram workspace.
// Every group goes all the way to out: the sums of two groups are joined mod q, never in the evaluation domain, so a group's integer
// stays within what P carries whatever the number of groups.
#include <algorithm>
#include <cstring>

#include "lambda_snark/batch.h"
#include "lsr_flavour.hpp"
#include "lsr_ring_mod_call.hpp"
#include "lsr_ring_mod_quadform_kernels.hpp"
#include "lsr_runtime.hpp"

namespace lsr {

constexpr size_t kModQuadMaxFamilies = 65534;                              // one grid axis; the last flag word is the shared c's
constexpr size_t kModQuadSharedFlag = 2 * kRingModGramFlagWords - 1;       // 32-bit flag word of a shared c: no chunk's clear reaches it
constexpr size_t kModQuadTargetGroups = 1024;   // workgroups a launch should reach before the pairs are left in one slice (4 per CU)
constexpr size_t kModQuadMinSlicePairs = 4;     // a slice pays 2 products and a c-hat_i load per row it touches
constexpr size_t kModQuadMaxSlices = 64;
static_assert((kModQuadMaxFamilies + 1) / 2 * 2 <= kModQuadSharedFlag, "a chunk's clear, in 64-bit words, leaves the shared word alone");
static_assert(2 * kModQuadMaxSlices <= 65535, "slices and primes share one grid axis");

// How the evaluation carries the second prime, by the compiler's resource report (profiles/r37_ring_mod_quadform_resource_usage.txt,
// DESIGN.md §5u): indexed ModParams keep 8 waves per SIMD in both flavours (56 and 57 VGPRs); the uniform branch costs the integer
// flavour three waves (96 VGPRs), one lane under both primes costs the FP64 flavour one (72) and the integer flavour four (108).
constexpr int kModQuadCarry = kQuadCarryIndex;

struct ModQuadCall {
    uint64_t* out;
    int32_t* status;
    const uint64_t *g, *c;
    size_t batch, r, c_rows;
    uint64_t offdiag, bound_g, bound_c;   // as the caller gave them: a bound of 0 = none
};

// what a call takes of P
struct ModQuadPlan {
    uint64_t bound_g, bound_c;   // resolved: none -> floor(q / 2)
    uint64_t weight;             // max(1, |w|) for the centred offdiag w: what an off-diagonal pair costs
    size_t group;                // pairs per group that P carries
};

static ModQuadPlan mod_quad_plan(const LsrRingMod& h, const ModQuadCall& c) {
    ModQuadPlan p{};
    const uint64_t half = h.q >> 1;
    p.bound_g = c.bound_g ? c.bound_g : half;
    p.bound_c = c.bound_c ? c.bound_c : half;
    p.weight = std::max<uint64_t>(1, c.offdiag <= half ? c.offdiag : h.q - c.offdiag);
    p.group = ring_mod_capacity_quadform(h.q, h.n, p.bound_g, p.bound_c) / p.weight;
    return p;
}

static unsigned mod_quad_threads(const LsrRingMod& h) { return std::min<unsigned>(kQuadThreads, std::max<unsigned>(64, h.n)); }

// slices of a launch over `count` pairs of `families` families, at most `cap`
static size_t mod_quad_slices(const LsrRingMod& h, size_t families, size_t count, size_t cap) {
    const size_t threads = mod_quad_threads(h), groups = 2 * ((h.n + threads - 1) / threads) * families;
    const size_t want = (kModQuadTargetGroups + groups - 1) / groups, most = (count + kModQuadMinSlicePairs - 1) / kModQuadMinSlicePairs;
    return std::max<size_t>(1, std::min({want, most, cap, kModQuadMaxSlices}));
}

// the checked lift (lsr_ring_mod_call.hpp) as the form takes it, one vector per family on the Gram workspace: `families` runs of `run`
// contiguous words, `src_fam` words apart, (CHECK) held against `bound` and q into flags[family] and (STORE) lifted to dst + family
// dst_fam for prime 0, half a workspace behind that for prime 1
template <bool CHECK, bool STORE>
static void quad_lift(const LsrRingMod& h, uint64_t* dst, const uint64_t* src, uint32_t* flags, size_t run, size_t families, size_t src_fam, size_t dst_fam,
                      uint64_t bound, hipStream_t s) {
    ring_mod_checked_lift<CHECK, STORE>(h, {dst, src, 1, families, run, 0, src_fam, 0, dst_fam, ring_mod_gram_words(), bound}, flags, s);
}

// One launch over the packed pairs [p0, p1) of `families` families for both primes (g-hat holds them from p0 on), and the sum of its
// slices: the canonical sums are in `sum` afterwards.
template <class A>
static void quad_evaluate(const LsrRingMod& h, uint64_t* sum, uint64_t* part, const uint64_t* ghat, const uint64_t* chat, const ModQuadCall& c, size_t p0,
                          size_t p1, size_t slices, size_t c_fam, size_t g_fam, size_t families, hipStream_t s) {
    constexpr int kCarry = kModQuadCarry;
    const unsigned threads = mod_quad_threads(h), runs = (h.n + threads - 1) / threads;
    const size_t half = ring_mod_gram_words();
    const ModQuadShape shape{(uint32_t)h.logn, (uint32_t)c.r, (uint32_t)p0, (uint32_t)p1, (uint32_t)slices, c_fam, g_fam, half};
    // (LiftSource::word on the host: the canonical residue of the centred offdiag)
    auto lifted = [&](int i) { return c.offdiag <= h.lift[i].half ? c.offdiag : c.offdiag + h.lift[i].rebase; };
    const ModQuadPrimes primes{{h.prime[0]->mod, h.prime[1]->mod}, {lifted(0), lifted(1)}};
    const unsigned grid_y = static_cast<unsigned>(kCarry == kQuadCarryLane ? slices : 2 * slices);
    hipLaunchKernelGGL((ring_mod_quadform_kernel<A, kCarry>), dim3(runs, grid_y, static_cast<unsigned>(families)), dim3(threads), 0, s, sum, part, ghat, chat,
                       shape, primes);
    if (slices > 1) {
        const ModQuadSumShape sums{(uint32_t)h.logn, (uint32_t)slices, half, {h.prime[0]->modulus, h.prime[1]->modulus}};
        hipLaunchKernelGGL(ring_mod_quadform_sum_kernel, dim3(runs, static_cast<unsigned>(families), 2), dim3(threads), 0, s, sum, part, sums);
    }
}

// The layout of a chunk in one prime's half of the workspace, in polynomials:
//   [c-hat: r per family, or r once for a shared c][g-hat: group per family][partials: slices per family, when slices > 1][sums: 1 per family]
// Pairs per group: what P carries (plan.group >= 1: mod_quad_call) and, for a family that does not fit whole, what the workspace
// leaves (polys >= r + 3: mod_quad_call).  Families per chunk: what the workspace holds of such groups, the chunks of a batch of equal
// size.
template <class A>
static void mod_quad_enqueue(const LsrRingMod& h, const ModQuadCall& c, hipStream_t s) {
    const ModQuadPlan plan = mod_quad_plan(h, c);
    const size_t n = h.n, half = ring_mod_gram_words(), polys = half >> h.logn, pairs = c.r * (c.r + 1) / 2;
    const bool shared = c.c_rows == 1;
    const size_t c_polys = shared ? 0 : c.r, rest = polys - (shared ? c.r : 0), g_fam = pairs * n, c_fam = c.r * n;
    uint64_t* const ws = h.gram_ws.ptr;
    uint32_t* const flags = ring_mod_gram_flags(h);
    auto transforms = [&](uint64_t* data, size_t count, bool inverse) { ring_mod_gram_transforms(h, data, count, inverse, s); };
    auto per_family = [&](size_t group, size_t sl) { return c_polys + group + (sl > 1 ? sl : 0) + 1; };

    size_t group = std::min(pairs, plan.group);
    size_t slices = mod_quad_slices(h, std::min(c.batch, kModQuadMaxFamilies), group, group);
    if (per_family(group, slices) > rest) slices = 1;
    size_t chunk_max = 1;
    if (per_family(group, slices) <= rest) {
        chunk_max = std::min(rest / per_family(group, slices), kModQuadMaxFamilies);
    } else {   // one family at a time, the workspace cuts its groups: room >= 2 polynomials for g-hat and the partials
        const size_t room = rest - c_polys - 1;
        slices = mod_quad_slices(h, 1, std::min(group, room - 1), room / 2);
        group = std::min(group, room - slices);
    }
    const size_t chunks = (c.batch + chunk_max - 1) / chunk_max, chunk = (c.batch + chunks - 1) / chunks;
    const bool one_group = group == pairs;
    uint64_t* const ghat = ws + (shared ? 1 : chunk) * c.r * n;
    uint64_t* const part = ghat + chunk * group * n;
    uint64_t* const sum = slices > 1 ? part + chunk * slices * n : part;

    if (shared) {
        zero_words_async(reinterpret_cast<uint64_t*>(flags + kModQuadSharedFlag - 1), 1, s);
        quad_lift<true, true>(h, ws, c.c, flags + kModQuadSharedFlag, c_fam, 1, 0, 0, plan.bound_c, s);
        transforms(ws, c.r, false);
    }
    for (size_t j0 = 0; j0 < c.batch; j0 += chunk) {
        const size_t now = std::min(chunk, c.batch - j0);
        const uint64_t* const gj = c.g + j0 * g_fam;
        zero_words_async(reinterpret_cast<uint64_t*>(flags), (now + 1) / 2, s);
        if (shared) {
            hipLaunchKernelGGL(ring_mod_quadform_spread_kernel, dim3(static_cast<unsigned>((now + kRingModThreads - 1) / kRingModThreads)), dim3(kRingModThreads),
                               0, s, flags, flags + kModQuadSharedFlag, static_cast<uint32_t>(now));
        } else {
            quad_lift<true, true>(h, ws, c.c + j0 * c_fam, flags, c_fam, now, c_fam, c_fam, plan.bound_c, s);
            transforms(ws, now * c.r, false);
        }
        if (!one_group) quad_lift<true, false>(h, nullptr, gj, flags, g_fam, now, g_fam, 0, plan.bound_g, s);
        for (size_t p0 = 0; p0 < pairs; p0 += group) {
            const size_t gnow = std::min(group, pairs - p0), run = gnow * n;
            for_bool(one_group, [&](auto check) { quad_lift<decltype(check)::value, true>(h, ghat, gj + p0 * n, flags, run, now, g_fam, run, plan.bound_g, s); });
            transforms(ghat, now * gnow, false);
            quad_evaluate<A>(h, sum, part, ghat, ws, c, p0, p0 + gnow, std::min(slices, gnow), shared ? 0 : c_fam, run, now, s);
            transforms(sum, now, true);
            ring_mod_gated_reduce(h, c.out + j0 * n, c.status + j0, sum, sum + half, flags, n, now, p0 > 0, s);
        }
    }
}

// One call on the device (caller validated the arguments) in the handle's bracket (ring_mod_call), on its Gram workspace
static void mod_quad_device(const LsrRingMod& h, const ModQuadCall& c, hipStream_t s) {
    ring_mod_call(h, s, true, [&] { for_ring_mod_flavour(h, [&](auto a) { mod_quad_enqueue<decltype(a)>(h, c, s); }); });
}

// host buffers through bounded device chunks of whole families on the first prime context's work stream (a shared c goes up once);
// status comes back with out
static void host_mod_quad(const LsrRingMod& h, const ModQuadCall& c) {
    const size_t n = h.n, g_words = c.r * (c.r + 1) / 2 * n, c_words = c.r * n;
    const bool shared = c.c_rows == 1;
    host_staged(*h.prime[0], c.batch, staging_chunk(c.batch, g_words + c_words + n),
                {staged_items(c.g, nullptr, g_words * 8), staged_items(c.c, nullptr, shared ? 0 : c_words * 8, c_words * 8), staged_items(nullptr, c.out, n * 8),
                 staged_items(nullptr, c.status, sizeof(int32_t))},
                [&](const StagedChunk& k, hipStream_t s) {
                    ModQuadCall d = c;
                    d.g = k.lane<const uint64_t>(0);
                    d.c = k.lane<const uint64_t>(1);
                    d.out = k.lane<uint64_t>(2);
                    d.status = k.lane<int32_t>(3);
                    d.batch = k.now;
                    d.c_rows = shared ? 1 : k.now;
                    mod_quad_device(h, d, s);
                });
}

}  // namespace lsr

// ------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------
namespace {

// The refusals of batch.h in its order, all before any device work.  Up to the bounds they read nothing of the handle but q.
int mod_quad_call(const char* where, const LsrRingMod* h, const lsr::ModQuadCall& c, bool device, void* stream) noexcept {
    if (!h || !c.out || !c.status || !c.g || !c.c) return lsr::abi_refuse(where, "NULL handle, buffer or status");
    if (c.r == 0) return lsr::abi_refuse(where, "r must be at least 1");
    if (c.c_rows != 1 && c.c_rows != c.batch)
        return lsr::abi_refuse(where, "c_rows must be 1 (one set of challenges for every family) or batch, got c_rows = " + std::to_string(c.c_rows) +
                                          ", batch = " + std::to_string(c.batch));
    if (c.r > LSR_RING_GRAM_MAX_VECTORS)
        return lsr::abi_refuse(where, "r = " + std::to_string(c.r) + " is above LSR_RING_GRAM_MAX_VECTORS (" + std::to_string(LSR_RING_GRAM_MAX_VECTORS) + ")");
    // in polynomials and then in bytes at the smallest ring (n = 2, 16 bytes a polynomial)
    size_t g_polys = 0, c_polys = 0, bytes = 0;
    const size_t pairs = c.r * (c.r + 1) / 2;
    const bool overflow = __builtin_mul_overflow(c.batch, pairs, &g_polys) || __builtin_mul_overflow(c.c_rows, c.r, &c_polys) ||
                          __builtin_mul_overflow(g_polys, (size_t)16, &bytes) || __builtin_mul_overflow(c_polys, (size_t)16, &bytes) ||
                          __builtin_mul_overflow(c.batch, (size_t)16, &bytes);
    if (overflow) return lsr::abi_refuse(where, "the sizes of g, c or out overflow size_t (batch, r, c_rows)");
    if (c.offdiag >= h->q)
        return lsr::abi_refuse(where, "offdiag = " + std::to_string(c.offdiag) + " is not a canonical word: the modulus is " + std::to_string(h->q));
    if (lsr::ring_mod_bounds_check(where, h->q, "bound_g", c.bound_g, "bound_c", c.bound_c) != 0) return -1;
    if (c.batch == 0) return 0;
    return lsr::abi_guarded(where, [&] {
        const size_t poly_bytes = (size_t)h->n * 8;
        // (at most 2080 polynomials of at most 2^20 bytes: no overflow)
        if (pairs * poly_bytes > LSR_RING_GRAM_MAX_FAMILY_BYTES)
            throw std::runtime_error("one family's g takes " + std::to_string(pairs * poly_bytes) + " bytes: above LSR_RING_GRAM_MAX_FAMILY_BYTES (" +
                                     std::to_string((size_t)LSR_RING_GRAM_MAX_FAMILY_BYTES) + ")");
        const lsr::ModQuadPlan p = lsr::mod_quad_plan(*h, c);
        if (p.group == 0)
            throw std::runtime_error("the form is cubic in its operands and q = " + std::to_string(h->q) + ", n = " + std::to_string(h->n) + " with bound_g = " +
                                     std::to_string(c.bound_g) + ", bound_c = " + std::to_string(c.bound_c) + " (0 states none) carries " +
                                     std::to_string(lsr::ring_mod_capacity_quadform(h->q, h->n, p.bound_g, p.bound_c)) +
                                     " triple products in one sum (lsr_ring_mod_capacity_quadform) where a pair weighted by offdiag takes " +
                                     std::to_string(p.weight) + ": state a bound_c on the challenges, or take lsr_ring_mod_mul_batch per pair (c_i c_l), scale the "
                                     "off-diagonal products by offdiag mod q and sum with lsr_ring_mod_dot_batch against g, which reduces mod q between the two "
                                     "products");
        const size_t polys = lsr::ring_mod_gram_words() >> h->logn;
        if (c.r + 3 > polys)
            throw std::runtime_error("r = " + std::to_string(c.r) + " challenges need a workspace of r + 3 polynomials per prime (the transformed c, one of g, one "
                                     "partial, one sum) even one pair at a time; it holds " + std::to_string(polys) +
                                     " at this ring degree (LAMBDA_SNARK_NTT_CHUNK_MIB sets the workspace size)");
        size_t out_bytes = 0, g_bytes = 0, c_bytes = 0;
        if (__builtin_mul_overflow(c.batch, poly_bytes, &out_bytes) || __builtin_mul_overflow(c.batch * pairs, poly_bytes, &g_bytes) ||
            __builtin_mul_overflow(c.c_rows * c.r, poly_bytes, &c_bytes))
            throw std::runtime_error("the sizes of g, c or out overflow size_t at this ring degree");
        lsr::require_outputs_apart({"out", c.out, out_bytes}, {"status", c.status, c.batch * sizeof(int32_t)}, {{"g", c.g, g_bytes}, {"c", c.c, c_bytes}});
        lsr::require_device();
        lsr::DeviceGuard guard(h->device);
        if (device) lsr::mod_quad_device(*h, c, static_cast<hipStream_t>(stream));
        else lsr::host_mod_quad(*h, c);
    });
}

}  // namespace

extern "C" {

size_t lsr_ring_mod_capacity_quadform(uint64_t q, uint32_t n, uint64_t bound_g, uint64_t bound_c) noexcept {
    try {
        return lsr::ring_mod_capacity_quadform(q, n, bound_g, bound_c);
    } catch (...) {
        return 0;
    }
}

int lsr_ring_mod_quadform_batch(const LsrRingMod* h, uint64_t* out, int32_t* status, const uint64_t* g, const uint64_t* c, size_t batch, size_t r,
                                size_t c_rows, uint64_t offdiag, uint64_t bound_g, uint64_t bound_c) noexcept {
    return mod_quad_call("lsr_ring_mod_quadform_batch", h, {out, status, g, c, batch, r, c_rows, offdiag, bound_g, bound_c}, false, nullptr);
}
int lsr_ring_mod_quadform_batch_device(const LsrRingMod* h, uint64_t* d_out, int32_t* d_status, const uint64_t* d_g, const uint64_t* d_c, size_t batch,
                                       size_t r, size_t c_rows, uint64_t offdiag, uint64_t bound_g, uint64_t bound_c, void* stream) noexcept {
    return mod_quad_call("lsr_ring_mod_quadform_batch_device", h, {d_out, d_status, d_g, d_c, batch, r, c_rows, offdiag, bound_g, bound_c}, true, stream);
}

}  // extern "C"

#ifdef LSR_RING_MOD_QUADFORM_REPORT
// resource-report builds only: every way of carrying the second prime, for both flavours
namespace lsr {
#define LSR_QUAD_INSTANCE(A, C) \
    template __global__ void ring_mod_quadform_kernel<A, C>(uint64_t*, uint64_t*, const uint64_t*, const uint64_t*, ModQuadShape, ModQuadPrimes);
LSR_QUAD_INSTANCE(ArithF64, kQuadCarryIndex)
LSR_QUAD_INSTANCE(ArithF64, kQuadCarryBranch)
LSR_QUAD_INSTANCE(ArithF64, kQuadCarryLane)
LSR_QUAD_INSTANCE(ArithU64, kQuadCarryIndex)
LSR_QUAD_INSTANCE(ArithU64, kQuadCarryBranch)
LSR_QUAD_INSTANCE(ArithU64, kQuadCarryLane)
#undef LSR_QUAD_INSTANCE
}  // namespace lsr
#endif
