// What the Gram calls of a context (lsr_ring_gram.hip) and of a ring handle under an arbitrary modulus
// (lsr_ring_mod_gram.hip, §5r) share on the host: the count of outputs, the grid limit and the checks of a shape that read neither a
// context nor a handle.  Host code only.
#pragma once
#include <string>

#include "lambda_snark/batch.h"
#include "lsr_ring_gram_kernels.hpp"
#include "lsr_runtime.hpp"

namespace lsr {

constexpr size_t kGramMaxGridZ = 65535;
static_assert((LSR_RING_GRAM_MAX_VECTORS / 2) * (LSR_RING_GRAM_MAX_VECTORS / 2) <= 65535, "the block pairs of one family are one grid axis");

// packed: the upper triangle i <= l of the symmetric and the symmetrised forms
inline size_t gram_outputs(size_t ra, size_t rb, bool packed) { return packed ? ra * (ra + 1) / 2 : ra * rb; }

// The checks of a shape in the documented order, after the NULL checks: -1 and a message, 0 to go on.  has_b: the call has a second
// operand (the cross and the symmetrised forms); sym2: the symmetrised form.
inline int ring_gram_shape_check(const char* where, bool has_b, size_t batch, size_t ra, size_t rb, size_t width, bool sym2) {
    if (ra == 0 || width == 0 || (has_b && rb == 0)) return abi_refuse(where, "ra, rb and width must be at least 1");
    if (!has_b && rb != ra)
        return abi_refuse(where, "the symmetric form (b == NULL) takes rb == ra, got ra = " + std::to_string(ra) + ", rb = " + std::to_string(rb));
    if (ra > LSR_RING_GRAM_MAX_VECTORS || rb > LSR_RING_GRAM_MAX_VECTORS)
        return abi_refuse(where, "ra = " + std::to_string(ra) + ", rb = " + std::to_string(rb) + ": above LSR_RING_GRAM_MAX_VECTORS (" +
                                     std::to_string(LSR_RING_GRAM_MAX_VECTORS) + ")");
    if (width > LSR_RING_DOT_MAX_TERMS)
        return abi_refuse(where, "width = " + std::to_string(width) + " is above LSR_RING_DOT_MAX_TERMS (" + std::to_string(LSR_RING_DOT_MAX_TERMS) + ")");
    // every product a shape takes, in polynomials and then in bytes at the smallest ring (n = 2, 16 bytes a polynomial)
    size_t vecs = 0, a_polys = 0, b_polys = 0, g_polys = 0, bytes = 0;
    const size_t outs = gram_outputs(ra, rb, !has_b || sym2);
    const bool overflow = __builtin_mul_overflow(batch, ra, &vecs) || __builtin_mul_overflow(vecs, width, &a_polys) ||
                          __builtin_mul_overflow(batch, rb, &vecs) || __builtin_mul_overflow(vecs, width, &b_polys) ||
                          __builtin_mul_overflow(batch, outs, &g_polys) || __builtin_mul_overflow(a_polys, (size_t)16, &bytes) ||
                          __builtin_mul_overflow(b_polys, (size_t)16, &bytes) || __builtin_mul_overflow(g_polys, (size_t)16, &bytes);
    if (overflow) return abi_refuse(where, "the sizes of a, b or g overflow size_t (batch, ra, rb, width)");
    return 0;
}

}  // namespace lsr
