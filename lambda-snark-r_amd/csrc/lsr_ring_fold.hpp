// What the folds of a context (lsr_ring_fold.hip) and of a ring handle under an arbitrary modulus
// (lsr_ring_mod_fold.hip, §5s) share on the host: the counts of a shape and the checks of it that read neither a context nor a
// handle.  Host code only.
#pragma once
#include <string>

#include "lambda_snark/batch.h"
#include "lsr_runtime.hpp"

namespace lsr {

struct FoldCounts {
    size_t vectors = 0, v_polys = 0, p_polys = 0, out_polys = 0;   // (outputs - 1) term_stride + terms; and the polynomials of v, p, out
};

// The checks of a shape in the documented order, after the NULL checks: -1 and a message, 1 for the empty call (a no-op), 0 to go on.
inline int ring_fold_shape_check(const char* where, size_t outputs, size_t terms, size_t ts, size_t width, FoldCounts& k) {
    if (terms == 0) return abi_refuse(where, "terms must be at least 1");
    if (outputs == 0 || width == 0) return 1;
    if (terms > LSR_RING_DOT_MAX_TERMS)
        return abi_refuse(where, "terms = " + std::to_string(terms) + " is above LSR_RING_DOT_MAX_TERMS (" + std::to_string(LSR_RING_DOT_MAX_TERMS) + ")");
    if (width > LSR_RING_FOLD_MAX_WIDTH)
        return abi_refuse(where, "width = " + std::to_string(width) + " is above LSR_RING_FOLD_MAX_WIDTH (" + std::to_string(LSR_RING_FOLD_MAX_WIDTH) + ")");
    // every product a shape takes, in polynomials and then in bytes at the smallest ring (n = 2, 16 bytes a polynomial)
    size_t span = 0;
    const bool overflow = __builtin_mul_overflow(outputs - 1, ts, &span) || __builtin_add_overflow(span, terms, &k.vectors) ||
                          __builtin_mul_overflow(k.vectors, width, &k.v_polys) || __builtin_mul_overflow(outputs, terms, &k.p_polys) ||
                          __builtin_mul_overflow(outputs, width, &k.out_polys) || __builtin_mul_overflow(k.v_polys, (size_t)16, &span) ||
                          __builtin_mul_overflow(k.p_polys, (size_t)16, &span) || __builtin_mul_overflow(k.out_polys, (size_t)16, &span);
    if (overflow) return abi_refuse(where, "the sizes of v, p or out overflow size_t (outputs, terms, term_stride, width)");
    return 0;
}

}  // namespace lsr
