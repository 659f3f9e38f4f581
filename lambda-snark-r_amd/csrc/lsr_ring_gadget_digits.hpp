// The balanced base-2^b digits of a ring element's words (batch.h "gadget decomposition") as every kernel that extracts
// them sees them: the parameters of (b, D) under a modulus, the host rules that admit them, and the two device functions that take a
// word to one digit.  Shared by lsr_ring_gadget_kernels.hpp (a context's prime) and lsr_ring_mod_matvec_kernels.hpp (a ring handle's q,
// any q >= 2).
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

namespace lsr {

// (b, D) and what the host derives from them and q.  With B = 2^b: off = B/2 in each of the D digit positions.  A digit fits 32 bits
// (b <= 32), so its arithmetic is 32-bit; q itself travels beside this struct (ModParams in the tile kernel).
struct GadgetParams {
    uint64_t off;
    uint64_t half_q;         // floor(q / 2): the largest word that is its own centred representative
    uint32_t digit_mask;     // B - 1
    uint32_t half_base;      // B / 2
    uint32_t base_log2, digits;
};

// B^D as a 128-bit integer (b D <= 64) and off = B/2 in every digit position
inline unsigned __int128 gadget_span(unsigned b, uint64_t digits) { return (unsigned __int128)1 << (b * digits); }
inline unsigned __int128 gadget_offset(unsigned b, uint64_t digits) {
    return ((unsigned __int128)1 << (b - 1)) * ((gadget_span(b, digits) - 1) / (((unsigned __int128)1 << b) - 1));
}

// the rules of batch.h that do not read q
inline bool gadget_shape_ok(unsigned b, uint64_t digits) { return b >= 2 && b <= 32 && digits >= 1 && digits <= 64 / b; }

inline bool gadget_admissible(uint64_t q, unsigned b, uint64_t digits) {
    if (!gadget_shape_ok(b, digits) || q < 2) return false;
    const unsigned __int128 off = gadget_offset(b, digits);
    return ((uint64_t)1 << (b - 1)) <= q / 2 && (q - 1) / 2 <= off && q / 2 <= gadget_span(b, digits) - 1 - off;
}

inline GadgetParams gadget_params(uint64_t q, unsigned b, uint64_t digits) {
    GadgetParams g{};
    g.half_q = q / 2;
    g.off = (uint64_t)gadget_offset(b, digits);   // below B^D <= 2^64
    g.digit_mask = (uint32_t)(((uint64_t)1 << b) - 1);
    g.half_base = 1u << (b - 1);
    g.base_log2 = b;
    g.digits = (uint32_t)digits;
    return g;
}

// u = centred(x) + off for a canonical x, in wrapping 64-bit arithmetic: 0 <= u < B^D <= 2^64 for an admissible (b, D)
__device__ __forceinline__ uint64_t gadget_shifted(uint64_t x, uint64_t q, const GadgetParams& g) { return x + g.off - (x > g.half_q ? q : 0ull); }
// digit d of the word behind u, as the canonical residue mod q of z_d = ((u >> b d) & (B - 1)) - B/2 in [-B/2, B/2 - 1]
__device__ __forceinline__ uint64_t gadget_digit(uint64_t u, uint32_t shift, uint64_t q, const GadgetParams& g) {
    const uint32_t t = (uint32_t)(u >> shift) & g.digit_mask;
    const uint32_t z = t - g.half_base;                        // two's complement of z_d in 32 bits (b = 32: B/2 = 2^31)
    return (uint64_t)(int64_t)(int32_t)z + (t < g.half_base ? q : 0ull);
}

}  // namespace lsr
