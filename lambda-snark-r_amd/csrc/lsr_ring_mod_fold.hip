// Fold of ring vectors by ring-valued challenges in Z_q[X]/(X^n + 1) for ANY modulus q >= 2 (batch.h "fold under any modulus",
// DESIGN.md §5s): lsr_ntt_ring_fold_batch on a ring handle (LsrRingMod, lsr_ring_mod.hip), n <= 4096, with the bounds and the status of
// the Gram calls (lsr_ring_mod_gram.hip).  The caller states l-infinity bounds on the centred words of v and of p; the device verifies
// them and reports per output (status), and the terms are taken in groups of what P = p1 p2 carries under those bounds
// (ring_mod_capacity_product).  Per chunk of outputs and group of terms:
//   1. ring_mod_gram_lift_kernel: the group's challenges read once, lifted for both primes into the b-hat rows of the handle's
//      workspace, bound_p and range folded into the output's flag word;
//   2. launch_ntt forward in place on each prime's rows: one transform per challenge, shared by the `width` components;
//   3. ntt_tile_ring_mod_fold, one launch for both primes (lsr_ring_mod_fold_kernels.hpp): v re-based for the workgroup's prime as it
//      is loaded, the first prime's workgroups holding it against bound_v and q, the sums into the handle's workspace;
//   4. ring_mod_gram_reduce_kernel: CRT and reduction mod q into out (accumulating from the second group on), zeros where the
//      output's flags are set — whatever the earlier groups wrote — and status.
// The flags of a chunk are cleared once and only accumulate over its groups, so a violation a later group finds still leaves the whole
// output zero.  Where the challenge rows hold fewer transforms than a chunk of full groups needs, a small chunk takes shorter groups
// and a large one fewer outputs (mod_fold_enqueue).  An output too wide for the sums (width n above 2^22 words) is taken alone, its components in chunks; its flags are
// then completed by a check pass without stores before its first reduce.
// The workspace is the handle's, allocated by lsr_ring_mod_create: [2][chunk][n] sums, [2][bhat_rows][n] challenge transforms, and
// kRingModFoldFlagWords words of per-output flags behind them (ring_mod_workspace, lsr_ring_mod_call.hpp, which also holds the
// launchers of the lift and of the reduce).
#include <algorithm>
#include <cstring>

#include "lambda_snark/batch.h"
#include "lsr_flavour.hpp"
#include "lsr_ring_fold.hpp"
#include "lsr_ring_mod_call.hpp"
#include "lsr_ring_mod_fold_kernels.hpp"
#include "lsr_runtime.hpp"

namespace lsr {

static_assert(kRingModBhatMaxRows <= 2 * kRingModFoldFlagWords, "one flag word per output of a chunk: every output has a challenge row");
static_assert(kRingModBhatMaxRows <= 65535, "the outputs of a chunk are one grid axis");

// tiles per prime from which a launch counts as filling the device: 1024 workgroups over both primes, four to a compute unit
constexpr size_t kRingModFoldFillTiles = 512;

// Both primes in one launch, the prime as grid z: in this form the check costs no registers over ntt_tile_ring_fold, where a launch
// per prime with the check as a template argument costs the checking launch 20 to 34 VGPRs in the FP64 flavour and a wave
// (profiles/r35_ring_mod_fold_resource_usage.txt).
template <class A>
static void fold_tiles(const LsrRingMod& h, const RingModWorkspace& w, const uint64_t* v, const RingModFoldShape& shape, size_t outputs, hipStream_t s) {
    const unsigned tiles = static_cast<unsigned>((shape.total + kTile - 1) / kTile);
    RingModFoldPrimes<A> both;
    for (int i = 0; i < 2; ++i) {
        const NttContext& c = *h.prime[i];
        both.prime[i] = {w.sums[i], w.bhat[i], Flavour<A>::fwd(c), Flavour<A>::inv(c), c.mod, Flavour<A>::consts(c), h.lift[i]};
    }
    for_tile_log<1, 12>(h.logn, [&](auto t) {
        constexpr int LT = decltype(t)::value;
        hipLaunchKernelGGL((ntt_tile_ring_mod_fold<A, LT>), dim3(tiles, static_cast<unsigned>(outputs), 2), dim3(kThreads), 0, s, both, v, w.flags, shape);
    });
}

// The loop of a fold with the stage behind the tiles as `stage` (ModFoldCall, ModFoldStage: lsr_ring_mod_call.hpp)
template <class A>
static void mod_fold_enqueue(const LsrRingMod& h, const ModFoldCall& c, const ModFoldStage& stage, hipStream_t s) {
    const size_t n = h.n, vec = c.width * n;
    const uint64_t half = h.q >> 1, bound_v = c.bound_v ? c.bound_v : half, bound_p = c.bound_p ? c.bound_p : half;
    const size_t capacity = ring_mod_capacity_product(h.q, h.n, bound_v, bound_p);    // >= max_terms >= 1
    const RingModWorkspace w = ring_mod_workspace(h);
    // An output wider than the sums goes alone, `wmax` components at a time.  Else a chunk holds whole outputs, as many as the sums
    // hold, and its groups as many terms as P carries; where the challenge rows do not hold that many transforms, a chunk that fills
    // the device (kRingModFoldFillTiles tiles per prime) keeps its full groups and takes fewer outputs, and a smaller one keeps its
    // outputs and takes shorter groups — few workgroups walking long sums one term at a time is the slower of the two.
    const size_t wmax = std::min(c.width, h.chunk);
    const bool whole = wmax == c.width;
    const size_t full_group = std::min({c.terms, capacity, h.bhat_rows});
    const size_t tiles = (vec + kTile - 1) / kTile, fill = (kRingModFoldFillTiles + tiles - 1) / tiles;
    const size_t want = whole ? std::min({c.outputs, h.chunk / c.width, std::max(h.bhat_rows / full_group, fill)}) : 1;
    const size_t group_max = std::min(full_group, std::max<size_t>(1, h.bhat_rows / want));
    const size_t chunk = std::min(want, h.bhat_rows / group_max);
    for (size_t j0 = 0; j0 < c.outputs; j0 += chunk) {
        const size_t now = std::min(chunk, c.outputs - j0);
        const uint64_t* const vj = c.v + j0 * c.ts * vec;
        const uint64_t* const pj = c.p + j0 * c.terms * n;
        zero_words_async(reinterpret_cast<uint64_t*>(w.flags), (now + 1) / 2, s);
        if (!whole && stage.flags_first) {   // (now == 1) the output's flags before its first reduce: its term vectors are contiguous in v
            ring_mod_check_pass(h, vj, w.flags, c.terms * vec, 1, 0, bound_v, s);
            ring_mod_check_pass(h, pj, w.flags, c.terms * n, 1, 0, bound_p, s);
        }
        for (size_t c0 = 0; c0 < c.width; c0 += wmax) {
            const size_t wnow = std::min(wmax, c.width - c0), words = wnow * n;
            for (size_t i0 = 0; i0 < c.terms; i0 += group_max) {
                const size_t group = std::min(group_max, c.terms - i0);
                // the group's challenges, contiguous per output, into the b-hat rows of both primes
                ring_mod_checked_lift<true, true>(h, {w.bhat[0], pj + i0 * n, 1, now, group * n, 0, c.terms * n, 0, group * n, h.bhat_rows * n, bound_p}, w.flags, s);
                for (int i = 0; i < 2; ++i) launch_ntt(*h.prime[i], w.bhat[i], now * group, false, s);
                const RingModFoldShape shape{words, (uint32_t)group, vec, c.ts * vec, h.q, bound_v};
                fold_tiles<A>(h, w, vj + i0 * vec + c0 * n, shape, now, s);
                stage.reduce({j0, now, c0, words, i0 == 0, i0 + group == c.terms}, w);
            }
        }
        if (stage.finish) stage.finish(j0, now, w);
    }
}

void ring_mod_fold_enqueue(const LsrRingMod& h, const ModFoldCall& c, const ModFoldStage& stage, hipStream_t s) {
    for_ring_mod_flavour(h, [&](auto a) { mod_fold_enqueue<decltype(a)>(h, c, stage, s); });
}

// One call on the device (caller validated the arguments) in the handle's bracket (ring_mod_call)
static void mod_fold_device(const LsrRingMod& h, const ModFoldCall& c, hipStream_t s) {
    const size_t n = h.n, vec = c.width * n;
    // out: [now][words] (one chunk of whole outputs, or one component range of one output), gated by the flags
    const ModFoldStage gated{[&](const ModFoldPiece& k, const RingModWorkspace& w) {
                                 ring_mod_gated_reduce(h, c.out + k.j0 * vec + k.c0 * n, c.status + k.j0, w.sums[0], w.sums[1], w.flags, k.words, k.now,
                                                       !k.first_group, s);
                             },
                             nullptr, true};
    ring_mod_call(h, s, false, [&] { ring_mod_fold_enqueue(h, c, gated, s); });
}

// host buffers through bounded device chunks on the first prime context's work stream: whole outputs with the span of vectors they
// read (each operand within the staging bound where one output's is; one output at a time otherwise); status comes back with out
static void host_mod_fold(const LsrRingMod& h, const ModFoldCall& c) {
    const size_t n = h.n, vec = c.width * n;
    host_staged(*h.prime[0], c.outputs, ring_mod_fold_staging_chunk(h, c),
                {staged_items(c.v, nullptr, c.ts * vec * 8, c.terms * vec * 8), staged_items(c.p, nullptr, c.terms * n * 8),
                 staged_items(nullptr, c.out, vec * 8), staged_items(nullptr, c.status, sizeof(int32_t))},
                [&](const StagedChunk& k, hipStream_t s) {
                    ModFoldCall d = c;
                    d.v = k.lane<const uint64_t>(0);
                    d.p = k.lane<const uint64_t>(1);
                    d.out = k.lane<uint64_t>(2);
                    d.status = k.lane<int32_t>(3);
                    d.outputs = k.now;
                    mod_fold_device(h, d, s);
                });
}

}  // namespace lsr

// ------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------
namespace {

// The refusals of batch.h in its order, all before any device work.  They read nothing of the handle but q and n.
int mod_fold_call(const char* where, const LsrRingMod* h, const lsr::ModFoldCall& c, bool device, void* stream) noexcept {
    if (!h || !c.out || !c.status || !c.v || !c.p) return lsr::abi_refuse(where, "NULL handle, buffer or status");
    lsr::FoldCounts k;
    const int rc = lsr::ring_fold_shape_check(where, c.outputs, c.terms, c.ts, c.width, k);
    if (rc != 0) return rc < 0 ? -1 : 0;
    if (lsr::ring_mod_bounds_check(where, h->q, "bound_v", c.bound_v, "bound_p", c.bound_p) != 0) return -1;
    return lsr::abi_guarded(where, [&] {
        if (h->n > lsr::kTile)
            throw std::runtime_error("n = " + std::to_string(h->n) + " is above 4096, where the fold has no fused form: lsr_ring_mod_lift_batch_device v and p for "
                                     "each prime, run lsr_ntt_ring_fold_batch_device on lsr_ring_mod_prime_context(h, 0) and (h, 1), and pass the two results to "
                                     "lsr_ring_mod_reduce_batch_device, with the terms in groups of at most max_terms (lsr_ring_mod_max_terms), every group "
                                     "after the first reduced with accumulate");
        const size_t poly_bytes = (size_t)h->n * 8;
        size_t v_bytes = 0, p_bytes = 0, out_bytes = 0;
        if (__builtin_mul_overflow(k.v_polys, poly_bytes, &v_bytes) || __builtin_mul_overflow(k.p_polys, poly_bytes, &p_bytes) ||
            __builtin_mul_overflow(k.out_polys, poly_bytes, &out_bytes))
            throw std::runtime_error("the sizes of v, p or out overflow size_t at this ring degree");
        lsr::require_outputs_apart({"out", c.out, out_bytes}, {"status", c.status, c.outputs * sizeof(int32_t)}, {{"v", c.v, v_bytes}, {"p", c.p, p_bytes}});
        lsr::require_device();
        lsr::DeviceGuard guard(h->device);
        if (device) lsr::mod_fold_device(*h, c, static_cast<hipStream_t>(stream));
        else lsr::host_mod_fold(*h, c);
    });
}

}  // namespace

extern "C" {

int lsr_ring_mod_fold_batch(const LsrRingMod* h, uint64_t* out, int32_t* status, const uint64_t* v, const uint64_t* p, size_t outputs, size_t terms,
                            size_t term_stride, size_t width, uint64_t bound_v, uint64_t bound_p) noexcept {
    return mod_fold_call("lsr_ring_mod_fold_batch", h, {out, status, v, p, outputs, terms, term_stride, width, bound_v, bound_p}, false, nullptr);
}
int lsr_ring_mod_fold_batch_device(const LsrRingMod* h, uint64_t* d_out, int32_t* d_status, const uint64_t* d_v, const uint64_t* d_p, size_t outputs,
                                   size_t terms, size_t term_stride, size_t width, uint64_t bound_v, uint64_t bound_p, void* stream) noexcept {
    return mod_fold_call("lsr_ring_mod_fold_batch_device", h, {d_out, d_status, d_v, d_p, outputs, terms, term_stride, width, bound_v, bound_p}, true, stream);
}

}  // extern "C"
