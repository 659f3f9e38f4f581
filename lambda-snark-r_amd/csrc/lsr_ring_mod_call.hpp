// The host call path shared by the operations on a ring handle under an arbitrary modulus (LsrRingMod; lsr_ring_mod.hip,
// lsr_ring_mod_matvec.hip, lsr_ring_mod_gram.hip, lsr_ring_mod_fold.hip, lsr_ring_mod_quadform.hip): the handle's
// counterpart of lsr_ring_call.hpp.  The bracket that keeps the handle's workspaces safe across streams and threads, the dispatch to the
// flavour of its prime contexts, the views of its two workspaces, the launchers of the checked lift and the gated reduce that every
// bounded call runs (lsr_ring_mod_kernels.hpp), and the refusals the bounded entry points have in common.  Host code only.
#pragma once
#include <functional>
#include <initializer_list>
#include <stdexcept>
#include <string>

#include "lsr_ring_call.hpp"
#include "lsr_ring_mod.hpp"

namespace lsr {

// (caller holds h.mutex) the Gram workspace, allocated once and never resized: lsr_ring_mod_gram_prepare, or the first eager call
inline void ring_mod_gram_workspace(const LsrRingMod& h) {
    if (!h.gram_ws.ptr) h.gram_ws.allocate(2 * ring_mod_gram_words() + kRingModGramFlagWords);
}

// The bracket of one call on the device (caller validated the arguments), ring_call's on the handle's own mutex and event: the Gram
// workspace allocated by the first call that needs it, the launches of `enqueue` on `s` behind the handle's previous call, and the
// event recorded behind them for the next one.  A capturing stream: no brackets (lsr_runtime.hpp, stream_is_capturing).
template <class Enqueue>
void ring_mod_call(const LsrRingMod& h, hipStream_t s, bool needs_gram_workspace, Enqueue&& enqueue) {
    std::lock_guard<std::mutex> lock(h.mutex);
    const bool capturing = stream_is_capturing(s);
    if (needs_gram_workspace) {
        // (an allocation inside the capture would not be part of the graph)
        if (capturing && !h.gram_ws.ptr) throw std::runtime_error(kWorkspaceBeforeCapture);
        ring_mod_gram_workspace(h);
    }
    if (!capturing) h.event.wait(s);
    enqueue();
    LSR_HIP(hipGetLastError());
    if (!capturing) h.event.record(s);
}

// f(A{}) for the flavour A of the prime contexts: FP64 unless the process forces the integer kernels, the same for both (one
// process-wide switch)
template <class F>
void for_ring_mod_flavour(const LsrRingMod& h, F&& f) {
    if (h.prime[0]->use_f64 != h.prime[1]->use_f64) throw std::runtime_error("the two prime contexts run different kernel flavours");
    if (h.prime[0]->use_f64) f(ArithF64{});
    else f(ArithU64{});
}

// The handle's workspace (n <= 4096) as its calls take it: per prime the sums of one chunk and the b-hat rows — transforms of a shared
// b or of a fold's challenges — and the 2 kRingModFoldFlagWords 32-bit flag words behind them: a fold's per-output flags, a bounded
// matrix product's per-vector flags.  Whoever holds the handle's mutex owns all of it.
struct RingModWorkspace {
    uint64_t* sums[2];
    uint64_t* bhat[2];
    uint32_t* flags;
};
inline RingModWorkspace ring_mod_workspace(const LsrRingMod& h) {
    uint64_t* const ws = h.ws.ptr;
    const size_t sums = h.chunk * h.n, rows = h.bhat_rows * h.n;   // (sums == kRingModSumWords)
    return {{ws, ws + sums}, {ws + 2 * sums, ws + 2 * sums + rows}, reinterpret_cast<uint32_t*>(ws + 2 * (sums + rows))};
}

// the per-family flag words behind the two halves of the Gram workspace
inline uint32_t* ring_mod_gram_flags(const LsrRingMod& h) { return reinterpret_cast<uint32_t*>(h.gram_ws.ptr + 2 * ring_mod_gram_words()); }

// `count` transforms in place for both primes: `data` in the first half of the Gram workspace, its twin half a workspace behind it
inline void ring_mod_gram_transforms(const LsrRingMod& h, uint64_t* data, size_t count, bool inverse, hipStream_t s) {
    for (int i = 0; i < 2; ++i) launch_ntt(*h.prime[i], data + i * ring_mod_gram_words(), count, inverse, s);
}

// One operand of a checked lift: `vectors` runs of `run` contiguous words per family, `families` families.  (CHECK) the words are held
// against q and `bound` into flags[family], (STORE) lifted to dst + family dst_fam + vector dst_vec for prime 0 and `half` words behind
// that for prime 1.
struct LiftLaunch {
    uint64_t* dst;
    const uint64_t* src;
    size_t vectors, families, run, src_vec, src_fam, dst_vec, dst_fam, half;
    uint64_t bound;
};

// (The launchers are templates — the check pass and the gated reduce on the handle's type, for nothing else — so that a translation
// unit instantiates the kernels of the launchers it calls and no others.)
template <bool CHECK, bool STORE>
void ring_mod_checked_lift(const LsrRingMod& h, const LiftLaunch& l, uint32_t* flags, hipStream_t s) {
    const bool vec = (reinterpret_cast<uintptr_t>(l.src) & 15u) == 0;
    const size_t items = vec ? l.run / 2 : l.run;
    const dim3 grid(static_cast<unsigned>(std::max<size_t>(1, std::min<size_t>((items + kRingModThreads - 1) / kRingModThreads, 1024))),
                    static_cast<unsigned>(l.vectors), static_cast<unsigned>(l.families));
    const GramLiftShape shape{l.run, l.src_vec, l.src_fam, l.dst_vec, l.dst_fam, l.half, h.q, l.bound};
    for_bool(vec, [&](auto v) {
        hipLaunchKernelGGL((ring_mod_gram_lift_kernel<decltype(v)::value, CHECK, STORE>), grid, dim3(kRingModThreads), 0, s, l.dst, l.src, flags, shape,
                           h.lift[0], h.lift[1]);
    });
}

// the `run` contiguous words of each of `families` families, `src_fam` words apart, held against q and `bound` into flags[family];
// nothing is stored
template <class Handle>
void ring_mod_check_pass(const Handle& h, const uint64_t* src, uint32_t* flags, size_t run, size_t families, size_t src_fam, uint64_t bound, hipStream_t s) {
    ring_mod_checked_lift<true, false>(h, {nullptr, src, 1, families, run, 0, src_fam, 0, 0, 0, bound}, flags, s);
}

// out: [families][words] from the two primes' sums r0 and r1, their families `words` apart as well, gated by the flags: zeros over a
// flagged family, and status
template <class Handle>
void ring_mod_gated_reduce(const Handle& h, uint64_t* out, int32_t* status, const uint64_t* r0, const uint64_t* r1, const uint32_t* flags, size_t words,
                           size_t families, bool accumulate, hipStream_t s) {
    const bool vec = (reinterpret_cast<uintptr_t>(out) & 15u) == 0;
    const size_t items = vec ? words / 2 : words;
    const dim3 grid(static_cast<unsigned>(std::max<size_t>(1, std::min<size_t>((items + kRingModThreads - 1) / kRingModThreads, 1024))),
                    static_cast<unsigned>(families));
    for_bool(vec, [&](auto v) {
        for_bool(accumulate, [&](auto acc) {
            hipLaunchKernelGGL((ring_mod_gram_reduce_kernel<decltype(v)::value, decltype(acc)::value>), grid, dim3(kRingModThreads), 0, s, out, status, r0, r1,
                               flags, words, words, h.rc, h.prime[1]->mod, h.pq);
        });
    });
}

// A fold on the handle (lsr_ring_mod_fold.hip) and the calls that run its loop with a reduce stage of their own
// (lsr_ring_mod_respond.hip): the arguments of one call, validated,
struct ModFoldCall {
    uint64_t* out;
    int32_t* status;
    const uint64_t *v, *p;
    size_t outputs, terms, ts, width;
    uint64_t bound_v, bound_p;   // as the caller gave them: 0 = none
};
// one group of terms of a chunk of outputs with its sums complete in the workspace: outputs [j0, j0 + now), `words` words of each
// from component c0 on (whole outputs, or one component range of one output taken alone)
struct ModFoldPiece {
    size_t j0, now, c0, words;
    bool first_group, last_group;
};
// and what runs behind the tiles.  reduce: every piece, in the loop's order; finish (may be empty): behind the last reduce of
// outputs [j0, j0 + now).  flags_first: an output taken alone has its flags completed by storeless check passes before its first
// reduce, as a reduce that gates its stores needs them.
struct ModFoldStage {
    std::function<void(const ModFoldPiece&, const RingModWorkspace&)> reduce;
    std::function<void(size_t j0, size_t now, const RingModWorkspace&)> finish;
    bool flags_first;
};
void ring_mod_fold_enqueue(const LsrRingMod& h, const ModFoldCall& c, const ModFoldStage& stage, hipStream_t s);   // lsr_ring_mod_fold.hip
// the outputs a host form stages at a time: whole outputs with the span of vectors they read, each operand within the staging bound
// where one output's is
inline size_t ring_mod_fold_staging_chunk(const LsrRingMod& h, const ModFoldCall& c) {
    const size_t bound = std::max<size_t>(1, staging_bytes() / ((size_t)h.n * 8));          // polynomials per staged operand
    const size_t fit_v = c.ts == 0 ? c.outputs : (bound / c.width > c.terms ? (bound / c.width - c.terms) / c.ts + 1 : 1);
    return std::max<size_t>(1, std::min({c.outputs, fit_v, bound / c.terms, bound / c.width}));
}

// batch.h's refusal of a stated bound above floor(q / 2), naming both bounds of the call (the second counts only where its operand
// is there): -1 refused, 0 to go on
inline int ring_mod_bounds_check(const char* where, uint64_t q, const char* name_a, uint64_t bound_a, const char* name_b, uint64_t bound_b,
                                 bool b_counts = true) {
    const uint64_t half = q >> 1;
    if (bound_a <= half && !(b_counts && bound_b > half)) return 0;
    return abi_refuse(where, std::string(name_a) + " = " + std::to_string(bound_a) + ", " + name_b + " = " + std::to_string(bound_b) +
                                 ": a bound is above floor(q / 2) = " + std::to_string(half) + " (0 states none)");
}

// batch.h's overlap refusals of a bounded call, in its order: out against every operand, status against every operand, status against
// out (an operand that is not there: NULL)
struct NamedRange {
    const char* name;
    const void* ptr;
    size_t bytes;
};
inline void require_outputs_apart(const NamedRange& out, const NamedRange& status, std::initializer_list<NamedRange> operands) {
    auto apart = [](const NamedRange& a, const NamedRange& b, const char* why) {
        if (ranges_overlap(a.ptr, a.bytes, b.ptr, b.bytes)) throw std::runtime_error(std::string(a.name) + " overlaps " + b.name + why);
    };
    for (const NamedRange* o : {&out, &status})
        for (const NamedRange& in : operands)
            if (in.ptr) apart(*o, in, ": the output must not share memory with an operand");
    apart(status, out, ": the two outputs must not share memory");
}

}  // namespace lsr
