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
// kRingModFoldFlagWords words of per-output flags behind them.
#include <algorithm>
#include <cstring>

#include "lambda_snark/batch.h"
#include "lsr_flavour.hpp"
#include "lsr_ring_call.hpp"
#include "lsr_ring_fold.hpp"
#include "lsr_ring_mod.hpp"
#include "lsr_ring_mod_fold_kernels.hpp"
#include "lsr_runtime.hpp"

namespace lsr {

static_assert(kRingModBhatMaxRows <= 2 * kRingModFoldFlagWords, "one flag word per output of a chunk: every output has a challenge row");
static_assert(kRingModBhatMaxRows <= 65535, "the outputs of a chunk are one grid axis");

// tiles per prime from which a launch counts as filling the device: 1024 workgroups over both primes, four to a compute unit
constexpr size_t kRingModFoldFillTiles = 512;

struct ModFoldCall {
    uint64_t* out;
    int32_t* status;
    const uint64_t *v, *p;
    size_t outputs, terms, ts, width;
    uint64_t bound_v, bound_p;   // as the caller gave them: 0 = none
};

// `families` runs of `run` contiguous words, `src_fam` words apart: checked against `bound` and q into flags[family] and (STORE)
// lifted to dst + family dst_fam for prime 0, `half` words behind that for prime 1
template <bool STORE>
static void fold_lift(const LsrRingMod& h, uint64_t* dst, const uint64_t* src, uint32_t* flags, size_t run, size_t families, size_t src_fam, size_t dst_fam,
                      size_t half, uint64_t bound, hipStream_t s) {
    const bool vec = (reinterpret_cast<uintptr_t>(src) & 15u) == 0;
    const size_t items = vec ? run / 2 : run;
    const dim3 grid(static_cast<unsigned>(std::max<size_t>(1, std::min<size_t>((items + kRingModThreads - 1) / kRingModThreads, 1024))), 1u,
                    static_cast<unsigned>(families));
    const GramLiftShape shape{run, 0, src_fam, 0, dst_fam, half, h.q, bound};
    for_bool(vec, [&](auto v) {
        hipLaunchKernelGGL((ring_mod_gram_lift_kernel<decltype(v)::value, true, STORE>), grid, dim3(kRingModThreads), 0, s, dst, src, flags, shape, h.lift[0],
                           h.lift[1]);
    });
}

// Both primes in one launch, the prime as grid z: in this form the check costs no registers over ntt_tile_ring_fold, where a launch
// per prime with the check as a template argument costs the checking launch 20 to 34 VGPRs in the FP64 flavour and a wave
// (profiles/r35_ring_mod_fold_resource_usage.txt).
template <class A>
static void fold_tiles(const LsrRingMod& h, uint64_t* const (&sums)[2], const uint64_t* const (&bhat)[2], const uint64_t* v, uint32_t* flags,
                       const RingModFoldShape& shape, size_t outputs, hipStream_t s) {
    const unsigned tiles = static_cast<unsigned>((shape.total + kTile - 1) / kTile);
    RingModFoldPrimes<A> both;
    for (int i = 0; i < 2; ++i) {
        const NttContext& c = *h.prime[i];
        both.prime[i] = {sums[i], bhat[i], Flavour<A>::fwd(c), Flavour<A>::inv(c), c.mod, Flavour<A>::consts(c), h.lift[i]};
    }
    for_tile_log<1, 12>(h.logn, [&](auto t) {
        constexpr int LT = decltype(t)::value;
        hipLaunchKernelGGL((ntt_tile_ring_mod_fold<A, LT>), dim3(tiles, static_cast<unsigned>(outputs), 2), dim3(kThreads), 0, s, both, v, flags, shape);
    });
}

// out: [outputs][words] (one chunk of whole outputs, or one component range of one output)
static void fold_reduce(const LsrRingMod& h, uint64_t* out, int32_t* status, const uint64_t* r0, const uint64_t* r1, const uint32_t* flags, size_t words,
                        size_t outputs, bool accumulate, hipStream_t s) {
    const bool vec = (reinterpret_cast<uintptr_t>(out) & 15u) == 0;
    const size_t items = vec ? words / 2 : words;
    const dim3 grid(static_cast<unsigned>(std::max<size_t>(1, std::min<size_t>((items + kRingModThreads - 1) / kRingModThreads, 1024))),
                    static_cast<unsigned>(outputs));
    for_bool(vec, [&](auto v) {
        for_bool(accumulate, [&](auto acc) {
            hipLaunchKernelGGL((ring_mod_gram_reduce_kernel<decltype(v)::value, decltype(acc)::value>), grid, dim3(kRingModThreads), 0, s, out, status, r0, r1,
                               flags, words, words, h.rc, h.prime[1]->mod, h.pq);
        });
    });
}

template <class A>
static void mod_fold_enqueue(const LsrRingMod& h, const ModFoldCall& c, hipStream_t s) {
    const size_t n = h.n, vec = c.width * n;
    const uint64_t half = h.q >> 1, bound_v = c.bound_v ? c.bound_v : half, bound_p = c.bound_p ? c.bound_p : half;
    const size_t capacity = ring_mod_capacity_product(h.q, h.n, bound_v, bound_p);    // >= max_terms >= 1
    uint64_t* const sums[2] = {h.ws.ptr, h.ws.ptr + h.chunk * n};
    uint64_t* const bhat_rw[2] = {h.ws.ptr + 2 * h.chunk * n, h.ws.ptr + (2 * h.chunk + h.bhat_rows) * n};
    const uint64_t* const bhat[2] = {bhat_rw[0], bhat_rw[1]};
    uint32_t* const flags = reinterpret_cast<uint32_t*>(h.ws.ptr + 2 * (h.chunk + h.bhat_rows) * n);
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
        zero_words_async(reinterpret_cast<uint64_t*>(flags), (now + 1) / 2, s);
        if (!whole) {   // (now == 1) the output's flags before its first reduce: its term vectors are contiguous in v
            fold_lift<false>(h, nullptr, vj, flags, c.terms * vec, 1, 0, 0, 0, bound_v, s);
            fold_lift<false>(h, nullptr, pj, flags, c.terms * n, 1, 0, 0, 0, bound_p, s);
        }
        for (size_t c0 = 0; c0 < c.width; c0 += wmax) {
            const size_t wnow = std::min(wmax, c.width - c0), words = wnow * n;
            for (size_t i0 = 0; i0 < c.terms; i0 += group_max) {
                const size_t group = std::min(group_max, c.terms - i0);
                fold_lift<true>(h, bhat_rw[0], pj + i0 * n, flags, group * n, now, c.terms * n, group * n, h.bhat_rows * n, bound_p, s);
                for (int i = 0; i < 2; ++i) launch_ntt(*h.prime[i], bhat_rw[i], now * group, false, s);
                const RingModFoldShape shape{words, (uint32_t)group, vec, c.ts * vec, h.q, bound_v};
                fold_tiles<A>(h, sums, bhat, vj + i0 * vec + c0 * n, flags, shape, now, s);
                fold_reduce(h, c.out + j0 * vec + c0 * n, c.status + j0, sums[0], sums[1], flags, words, now, i0 > 0, s);
            }
        }
    }
}

// One call on the device (caller validated the arguments): the handle's mutex and event as ring_mod_dot_device.
static void mod_fold_device(const LsrRingMod& h, const ModFoldCall& c, hipStream_t s) {
    std::lock_guard<std::mutex> lock(h.mutex);
    const bool capturing = stream_is_capturing(s);
    if (h.prime[0]->use_f64 != h.prime[1]->use_f64) throw std::runtime_error("the two prime contexts run different kernel flavours");
    if (!capturing) h.event.wait(s);
    if (h.prime[0]->use_f64) mod_fold_enqueue<ArithF64>(h, c, s);
    else mod_fold_enqueue<ArithU64>(h, c, s);
    LSR_HIP(hipGetLastError());
    if (!capturing) h.event.record(s);
}

// host buffers through bounded device chunks on the first prime context's work stream: whole outputs with the span of vectors they
// read (each operand within the staging bound where one output's is; one output at a time otherwise); status comes back with out
static void host_mod_fold(const LsrRingMod& h, const ModFoldCall& c) {
    const size_t n = h.n, vec = c.width * n;
    const size_t bound = std::max<size_t>(1, staging_bytes() / (n * 8));          // polynomials per staged operand
    const size_t fit_v = c.ts == 0 ? c.outputs : (bound / c.width > c.terms ? (bound / c.width - c.terms) / c.ts + 1 : 1);
    const size_t chunk = std::max<size_t>(1, std::min({c.outputs, fit_v, bound / c.terms, bound / c.width}));
    host_staged(*h.prime[0], c.outputs, chunk,
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
    const uint64_t half = h->q >> 1;
    if (c.bound_v > half || c.bound_p > half)
        return lsr::abi_refuse(where, "bound_v = " + std::to_string(c.bound_v) + ", bound_p = " + std::to_string(c.bound_p) + ": a bound is above floor(q / 2) = " +
                                          std::to_string(half) + " (0 states none)");
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
        const size_t status_bytes = c.outputs * sizeof(int32_t);
        lsr::require_apart(c.out, out_bytes, c.v, v_bytes, "out overlaps v: the output must not share memory with an operand");
        lsr::require_apart(c.out, out_bytes, c.p, p_bytes, "out overlaps p: the output must not share memory with an operand");
        lsr::require_apart(c.status, status_bytes, c.v, v_bytes, "status overlaps v: the output must not share memory with an operand");
        lsr::require_apart(c.status, status_bytes, c.p, p_bytes, "status overlaps p: the output must not share memory with an operand");
        lsr::require_apart(c.status, status_bytes, c.out, out_bytes, "status overlaps out: the two outputs must not share memory");
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
