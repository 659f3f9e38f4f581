// The sizing of the context's ring inner-product workspace (NttContext::ring_dot_scratch) and the flags of a sum taken in groups of
// terms through it, shared by the calls that use it:
// lsr_ring_dot.hip, lsr_ring_fold.hip (§5g) and lsr_ring_galois.hip (§5h).  Sizes are functions of n and of the process-wide chunk size alone.
#pragma once
#include <algorithm>

#include "lsr_ntt_kernels.hpp"
#include "lsr_runtime.hpp"

namespace lsr {

// Polynomials per workspace array.  n > 4096: three arrays are live between the passes of a chunk (the transformed a terms, the
// transformed b terms, the c chunk), so each gets a third of the Infinity Cache budget of a two-pass transform (ntt_chunk_bytes():
// 256 MiB -> 170 polynomials at n = 2^16).  n <= 4096: the same budget bounds the b-hat rows of a shared b, at most 4096 of them.
inline size_t ring_dot_chunk_polys(const NttContext& c) {
    const size_t polys = std::max<size_t>(1, (ntt_chunk_bytes() / 3) >> (c.logn + 3));
    return c.logn > kTileLog ? polys : std::min<size_t>(polys, 4096);
}
// Workspace words: n > 4096 — the a terms and the b terms (or b-hat rows) of one chunk; n <= 4096 — the b-hat rows.  A function of n
// (and of the process-wide chunk size) only, never of the batch or the terms.
inline size_t ring_dot_scratch_words(const NttContext& c) {
    return (c.logn > kTileLog ? 2 : 1) * ring_dot_chunk_polys(c) * c.degree;
}
// the flags of one launch of a sum taken in groups of terms: it starts the sums (first group) and / or finishes them (last group)
inline uint32_t ring_dot_flags(bool first, bool last) { return (first ? kRingDotFirst : 0u) | (last ? kRingDotLast : 0u); }

}  // namespace lsr
