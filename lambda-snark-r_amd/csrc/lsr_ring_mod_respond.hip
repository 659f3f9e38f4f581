// Masked responses of a Fiat-Shamir-with-aborts protocol in Z_q[X]/(X^n + 1) for ANY modulus q >= 2 (batch.h "responses under any
// modulus"): z_j = y_j + sum_i c_{j,i} s_{j term_stride + i} on a ring handle (LsrRingMod), n <= 4096, accepted only
// where the centred words of z_j stay within bound_z and all zero otherwise.  The loop is the fold's (ring_mod_fold_enqueue,
// lsr_ring_mod_fold.hip): its chunks of outputs, its groups of terms, the checked lift and the transforms of the challenges, and
// ntt_tile_ring_mod_fold.  Only the stage behind the tiles is this file's (lsr_ring_mod_respond_kernels.hpp):
//   ring_mod_respond_reduce_kernel   per group: CRT and reduction mod q into out — the first group adds y and holds it against q
//            and bound_y, every later group accumulates, the last holds the finished word against bound_z — all into the output's
//            flag word;
//   ring_mod_respond_finish_kernel   per chunk of outputs, behind its last reduce: status, and zeros over every flagged output.
// The reduce never gates its stores, so an output taken alone in component chunks needs no check pass in front: its flags are
// complete when the finish reads them, and the finish covers the whole output, the components of earlier chunks included.
#include <stdexcept>
#include <string>

#include "lambda_snark/batch.h"
#include "lsr_ring_fold.hpp"
#include "lsr_ring_mod_call.hpp"
#include "lsr_ring_mod_respond_kernels.hpp"
#include "lsr_runtime.hpp"

namespace lsr {

struct ModRespondCall {
    ModFoldCall fold;
    const uint64_t* y;            // NULL: no mask; may be fold.out
    uint64_t bound_y, bound_z;    // as the caller gave them: 0 = none
};

// grid x: a grid-stride run over an output's words, `per_lane` accesses a lane, capped at 1024 workgroups; grid y: the output
static dim3 respond_grid(size_t words, bool vec, size_t outputs, size_t per_lane = 1) {
    const size_t items = vec ? words / 2 : words, per_group = kRingModThreads * per_lane;
    return dim3(static_cast<unsigned>(std::max<size_t>(1, std::min<size_t>((items + per_group - 1) / per_group, 1024))), static_cast<unsigned>(outputs));
}
// Most workgroups of a finish read one flag word and return: few of them per output, eight stores a lane where the output is flagged
constexpr size_t kRespondFinishPerLane = 8;

static void mod_respond_device(const LsrRingMod& h, const ModRespondCall& c, hipStream_t s) {
    const ModFoldCall& f = c.fold;
    const size_t n = h.n, vec = f.width * n;
    const uint64_t half = h.q >> 1, bound_y = c.bound_y ? c.bound_y : half, bound_z = c.bound_z ? c.bound_z : half;
    // 16-byte accesses where out and y both allow them (every offset below is a multiple of n >= 2 words)
    const bool wide = ((reinterpret_cast<uintptr_t>(f.out) | reinterpret_cast<uintptr_t>(c.y)) & 15u) == 0;
    const ModFoldStage stage{
        [&](const ModFoldPiece& k, const RingModWorkspace& w) {
            const size_t at = k.j0 * vec + k.c0 * n;
            for_bool(wide, [&](auto v) {
                for_bool(k.first_group, [&](auto first) {
                    for_bool(k.last_group, [&](auto last) {
                        constexpr bool kFirst = decltype(first)::value;
                        hipLaunchKernelGGL((ring_mod_respond_reduce_kernel<decltype(v)::value, !kFirst, kFirst, decltype(last)::value>),
                                           respond_grid(k.words, wide, k.now), dim3(kRingModThreads), 0, s, f.out + at, c.y ? c.y + at : nullptr, w.sums[0],
                                           w.sums[1], w.flags, k.words, h.rc, h.prime[1]->mod, h.pq, bound_y, bound_z);
                    });
                });
            });
        },
        [&](size_t j0, size_t now, const RingModWorkspace& w) {
            const bool wide_out = (reinterpret_cast<uintptr_t>(f.out) & 15u) == 0;
            for_bool(wide_out, [&](auto v) {
                hipLaunchKernelGGL(ring_mod_respond_finish_kernel<decltype(v)::value>, respond_grid(vec, wide_out, now, kRespondFinishPerLane), dim3(kRingModThreads), 0, s,
                                   f.out + j0 * vec, f.status + j0, w.flags, vec);
            });
        },
        false};
    ring_mod_call(h, s, false, [&] { ring_mod_fold_enqueue(h, f, stage, s); });
}

// host buffers as the fold's (host_mod_fold): y one more lane, or out's lane going up as well where y is out
static void host_mod_respond(const LsrRingMod& h, const ModRespondCall& c) {
    const ModFoldCall& f = c.fold;
    const size_t n = h.n, vec = f.width * n;
    const bool in_place = c.y == f.out;
    host_staged(*h.prime[0], f.outputs, ring_mod_fold_staging_chunk(h, f),
                {staged_items(f.v, nullptr, f.ts * vec * 8, f.terms * vec * 8), staged_items(f.p, nullptr, f.terms * n * 8),
                 staged_items(in_place ? c.y : nullptr, f.out, vec * 8), staged_items(nullptr, f.status, sizeof(int32_t)),
                 staged_items(in_place ? nullptr : c.y, nullptr, c.y && !in_place ? vec * 8 : 0)},
                [&](const StagedChunk& k, hipStream_t s) {
                    ModRespondCall d = c;
                    d.fold.v = k.lane<const uint64_t>(0);
                    d.fold.p = k.lane<const uint64_t>(1);
                    d.fold.out = k.lane<uint64_t>(2);
                    d.fold.status = k.lane<int32_t>(3);
                    d.fold.outputs = k.now;
                    d.y = in_place ? d.fold.out : k.lane<const uint64_t>(4);   // (an absent lane: NULL)
                    mod_respond_device(h, d, s);
                });
}

}  // namespace lsr

// ------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------
namespace {

// The refusals of batch.h in its order — the fold's, y and the two further bounds joining at the bound check — all before any device
// work.  They read nothing of the handle but q and n.
int mod_respond_call(const char* where, const LsrRingMod* h, const lsr::ModRespondCall& c, bool device, void* stream) noexcept {
    const lsr::ModFoldCall& f = c.fold;
    if (!h || !f.out || !f.status || !f.v || !f.p) return lsr::abi_refuse(where, "NULL handle, buffer or status");
    lsr::FoldCounts k;
    const int rc = lsr::ring_fold_shape_check(where, f.outputs, f.terms, f.ts, f.width, k);
    if (rc != 0) return rc < 0 ? -1 : 0;
    const uint64_t half = h->q >> 1;
    const std::string bounds = "bound_y = " + std::to_string(c.bound_y) + ", bound_v = " + std::to_string(f.bound_v) + ", bound_p = " +
                               std::to_string(f.bound_p) + ", bound_z = " + std::to_string(c.bound_z);
    if (!c.y && c.bound_y != 0) return lsr::abi_refuse(where, bounds + ": y is NULL, so there is no mask for bound_y to bind (pass 0)");
    if (c.bound_y > half || f.bound_v > half || f.bound_p > half || c.bound_z > half)
        return lsr::abi_refuse(where, bounds + ": a bound is above floor(q / 2) = " + std::to_string(half) + " (0 states none)");
    return lsr::abi_guarded(where, [&] {
        if (h->n > lsr::kTile)
            throw std::runtime_error("n = " + std::to_string(h->n) + " is above 4096, where the response has no fused form: take the fold's composed route — "
                                     "lsr_ring_mod_lift_batch_device v and p for each prime, lsr_ntt_ring_fold_batch_device on "
                                     "lsr_ring_mod_prime_context(h, 0) and (h, 1), lsr_ring_mod_reduce_batch_device, with the terms in groups of at most "
                                     "max_terms (lsr_ring_mod_max_terms), every group after the first reduced with accumulate — then add y mod q and "
                                     "hold the sum with lsr_ntt_ring_linf_batch_device on lsr_ring_mod_coeff_context(h)");
        const size_t poly_bytes = (size_t)h->n * 8;
        size_t v_bytes = 0, p_bytes = 0, out_bytes = 0;
        if (__builtin_mul_overflow(k.v_polys, poly_bytes, &v_bytes) || __builtin_mul_overflow(k.p_polys, poly_bytes, &p_bytes) ||
            __builtin_mul_overflow(k.out_polys, poly_bytes, &out_bytes))
            throw std::runtime_error("the sizes of v, p or out overflow size_t at this ring degree");
        // y is out itself (in place) or apart from it; status is apart from everything
        const bool in_place = c.y == f.out;
        lsr::require_outputs_apart({"out", f.out, out_bytes}, {"status", f.status, f.outputs * sizeof(int32_t)},
                                   {{"y", in_place ? nullptr : c.y, out_bytes}, {"v", f.v, v_bytes}, {"p", f.p, p_bytes}});
        lsr::require_device();
        lsr::DeviceGuard guard(h->device);
        if (device) lsr::mod_respond_device(*h, c, static_cast<hipStream_t>(stream));
        else lsr::host_mod_respond(*h, c);
    });
}

}  // namespace

extern "C" {

int lsr_ring_mod_respond_batch(const LsrRingMod* h, uint64_t* out, int32_t* status, const uint64_t* y, const uint64_t* v, const uint64_t* p, size_t outputs,
                               size_t terms, size_t term_stride, size_t width, uint64_t bound_y, uint64_t bound_v, uint64_t bound_p,
                               uint64_t bound_z) noexcept {
    return mod_respond_call("lsr_ring_mod_respond_batch", h, {{out, status, v, p, outputs, terms, term_stride, width, bound_v, bound_p}, y, bound_y, bound_z}, false,
                            nullptr);
}
int lsr_ring_mod_respond_batch_device(const LsrRingMod* h, uint64_t* d_out, int32_t* d_status, const uint64_t* d_y, const uint64_t* d_v, const uint64_t* d_p,
                                      size_t outputs, size_t terms, size_t term_stride, size_t width, uint64_t bound_y, uint64_t bound_v, uint64_t bound_p,
                                      uint64_t bound_z, void* stream) noexcept {
    return mod_respond_call("lsr_ring_mod_respond_batch_device", h,
                            {{d_out, d_status, d_v, d_p, outputs, terms, term_stride, width, bound_v, bound_p}, d_y, bound_y, bound_z}, true, stream);
}

}  // extern "C"
