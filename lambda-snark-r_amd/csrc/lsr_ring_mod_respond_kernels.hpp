// The reduce stage of a masked response z = y + sum c s under an arbitrary modulus q (lsr_ring_mod_respond.hip, batch.h "responses
// under any modulus").  Everything in front of it is the fold's (lsr_ring_mod_fold_kernels.hpp); these two kernels
// take the place of ring_mod_gram_reduce_kernel (lsr_ring_mod_kernels.hpp):
//   ring_mod_respond_reduce_kernel   CRT and reduction mod q of one group's sums into out, the mask y added with the first group
//            and held against q and bound_y, the finished word held against bound_z with the last group.  What it finds goes into the
//            output's flag word — the two bits of ring_mod_gram_lift_kernel and a third, kRespondFlagRejected — folded the same
//            way: a lane ORs its bits, a wave ballots once per bit, at most one atomic OR per wave.  It never zeroes: whether an
//            output is rejected is known only when every workgroup of its last reduce has finished.
//   ring_mod_respond_finish_kernel   launched behind the last reduce of a chunk of outputs: status from the complete flags, and zeros
//            over every word of a flagged output; the workgroups of an unflagged output return at once.
// out and y carry no __restrict__: y may be out itself (a lane reads its words of y before it writes them to out, and no lane touches
// another lane's).  VEC: out and y both 16-byte aligned — 16 bytes per lane and access; the sums always are.  words is even (a
// multiple of n >= 2).
#pragma once

#include "lsr_ring_mod_kernels.hpp"

namespace lsr {

constexpr uint32_t kRespondFlagRejected = 4u;   // beside kGramFlagOverBound and kGramFlagNotBelowQ

// out, y: [outputs][words], r0 / r1: the outputs `words` apart as well (y NULL: no mask; read with FIRST alone).  Grid: x = runs of an
// output's words (grid-stride), y = output.  ACC: the word is added to what out holds; FIRST: y's word is added and checked; LAST:
// the finished word's centred magnitude is held against bound_z.  (A word of y at or above q adds to anything: the output is
// flagged and the finish writes zeros over it.)
template <bool VEC, bool ACC, bool FIRST, bool LAST>
__global__ void __launch_bounds__(kRingModThreads) ring_mod_respond_reduce_kernel(uint64_t* out_all, const uint64_t* y_all, const uint64_t* __restrict__ r0,
                                                                                   const uint64_t* __restrict__ r1, uint32_t* flags, size_t words,
                                                                                   RingModConsts rc, ModParams p2, ModParams pq, uint64_t bound_y,
                                                                                   uint64_t bound_z) {
    static_assert(ACC != FIRST, "the first group stores (over y, where y is out), every later one accumulates");
    // an output that already holds a word >= q has its status: its arithmetic may go (workgroup-uniform up to what another wave has
    // raised meanwhile, and there is no barrier below)
    if (flags[blockIdx.y] & kGramFlagNotBelowQ) return;
    const size_t stride = (size_t)gridDim.x * kRingModThreads, first = (size_t)blockIdx.x * kRingModThreads + threadIdx.x;
    uint64_t* const out = out_all + blockIdx.y * words;
    const bool masked = FIRST && y_all != nullptr;
    const uint64_t* const y = masked ? y_all + blockIdx.y * words : nullptr;
    const uint64_t* const a = r0 + blockIdx.y * words;
    const uint64_t* const b = r1 + blockIdx.y * words;
    const uint64_t q = pq.q, half = q >> 1;
    uint32_t bits = 0;
    // old: what out holds (ACC) or y's word (FIRST and masked)
    auto word = [&](uint64_t s0, uint64_t s1, uint64_t old) {
        uint64_t w = ring_mod_reduce_word(s0, s1, rc, p2, pq);
        if constexpr (FIRST) {
            if (masked) {
                const uint64_t mag = old <= half ? old : q - old;
                bits |= old >= q ? kGramFlagNotBelowQ : (mag > bound_y ? kGramFlagOverBound : 0u);
                w = ring_mod_add(old, w, q);
            }
        }
        if constexpr (ACC) w = ring_mod_add(old, w, q);
        if constexpr (LAST) {
            const uint64_t mag = w <= half ? w : q - w;
            bits |= mag > bound_z ? kRespondFlagRejected : 0u;
        }
        return w;
    };
    if constexpr (VEC) {
        for (size_t e = first; e < (words >> 1); e += stride) {
            const ulonglong2 s0 = reinterpret_cast<const ulonglong2*>(a)[e], s1 = reinterpret_cast<const ulonglong2*>(b)[e];
            ulonglong2 old = make_ulonglong2(0, 0);
            if constexpr (ACC) old = reinterpret_cast<const ulonglong2*>(out)[e];
            else if (masked) old = reinterpret_cast<const ulonglong2*>(y)[e];
            ulonglong2 v;
            v.x = word(s0.x, s1.x, old.x);
            v.y = word(s0.y, s1.y, old.y);
            reinterpret_cast<ulonglong2*>(out)[e] = v;
        }
    } else {
        for (size_t e = first; e < words; e += stride) {
            const uint64_t old = ACC ? out[e] : (masked ? y[e] : 0);
            out[e] = word(a[e], b[e], old);
        }
    }
    if constexpr (FIRST || LAST) {
        // every lane that did not leave at the top arrives here: the ballots see whole waves
        const uint32_t wave_bits = (__ballot(bits & kGramFlagOverBound) ? kGramFlagOverBound : 0u) | (__ballot(bits & kGramFlagNotBelowQ) ? kGramFlagNotBelowQ : 0u) |
                                   (__ballot(bits & kRespondFlagRejected) ? kRespondFlagRejected : 0u);
        if (wave_bits && (threadIdx.x & (warpSize - 1)) == 0) atomicOr(&flags[blockIdx.y], wave_bits);
    }
}

// status[output] from its complete flags — -1 over 0 over LSR_RING_RESPOND_REJECTED over 1 — by lane 0 of the output's first workgroup,
// and zeros over the `words` words of a flagged output.  out: [outputs][words].  Grid as above.
template <bool VEC>
__global__ void __launch_bounds__(kRingModThreads) ring_mod_respond_finish_kernel(uint64_t* __restrict__ out_all, int32_t* __restrict__ status,
                                                                                   const uint32_t* __restrict__ flags, size_t words) {
    const size_t stride = (size_t)gridDim.x * kRingModThreads, first = (size_t)blockIdx.x * kRingModThreads + threadIdx.x;
    const uint32_t bits = flags[blockIdx.y];
    if (first == 0) status[blockIdx.y] = (bits & kGramFlagNotBelowQ) ? -1 : (bits & kGramFlagOverBound) ? 0 : (bits & kRespondFlagRejected) ? 2 : 1;
    if (!bits) return;
    uint64_t* const out = out_all + blockIdx.y * words;
    if constexpr (VEC) {
        for (size_t e = first; e < (words >> 1); e += stride) reinterpret_cast<ulonglong2*>(out)[e] = make_ulonglong2(0, 0);
    } else {
        for (size_t e = first; e < words; e += stride) out[e] = 0;
    }
}

}  // namespace lsr
