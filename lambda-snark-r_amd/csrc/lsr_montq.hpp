// Montgomery arithmetic modulo any odd q < 2^64 (host and device): the Lagrange prove path (lsr_lagrange_kernels.hpp) and the
// witness-polynomial proofs (lsr_simple_kernels.hpp).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace lsr {

// ---- Montgomery arithmetic modulo any odd q < 2^64 (host and device) --------------------------------------------------------
// qinv = -q^-1 mod 2^64; r1, r2, r3 = 2^64, 2^128, 2^192 mod q.  Every value named "canonical" is < q.
struct MontQ {
    uint64_t q, qinv, r1, r2, r3;
};

__host__ __device__ inline uint64_t mq_mulhi(uint64_t a, uint64_t b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// (hi:lo) 2^-64 mod q, canonical, for hi:lo < q 2^64.  With t = lo qinv, lo + (t q mod 2^64) is 0 or exactly 2^64, so
// (hi:lo + t q) / 2^64 = hi + mulhi(t, q) + [lo != 0] < 2q: one subtraction, where a carry out of 64 bits means >= q.
__host__ __device__ inline uint64_t mq_redc(uint64_t hi, uint64_t lo, const MontQ& M) {
    const uint64_t t = lo * M.qinv;
    const uint64_t th = mq_mulhi(t, M.q);
    uint64_t s = hi + th;
    bool carry = s < hi;
    const uint64_t c = lo != 0 ? 1u : 0u;
    s += c;
    carry |= s < c;
    if (carry || s >= M.q) s -= M.q;
    return s;
}
// a b 2^-64 mod q, canonical: needs a < q or b < q (then a b < q 2^64)
__host__ __device__ inline uint64_t mq_mul(uint64_t a, uint64_t b, const MontQ& M) { return mq_redc(mq_mulhi(a, b), a * b, M); }
__host__ __device__ inline uint64_t mq_add(uint64_t a, uint64_t b, const MontQ& M) {   // a, b canonical
    uint64_t s = a + b;
    if (s < a || s >= M.q) s -= M.q;
    return s;
}
__host__ __device__ inline uint64_t mq_sub(uint64_t a, uint64_t b, const MontQ& M) {   // a, b canonical
    return a >= b ? a - b : a - b + M.q;
}
__host__ __device__ inline uint64_t mq_to(uint64_t x, const MontQ& M) { return mq_mul(x, M.r2, M); }   // x 2^64 (any 64-bit x)
__host__ __device__ inline uint64_t mq_canon(uint64_t x, const MontQ& M) { return mq_redc(0, mq_mul(x, M.r2, M), M); }   // x mod q

// the constants of an odd q (host)
inline MontQ make_mont(uint64_t q) {
    MontQ M{};
    M.q = q;
    uint64_t inv = q;                       // Newton: q^-1 mod 2^64 (q odd; 5 steps from 3 correct bits)
    for (int i = 0; i < 5; ++i) inv *= 2 - q * inv;
    M.qinv = 0 - inv;
    M.r1 = (uint64_t)(((unsigned __int128)1 << 64) % q);
    M.r2 = (uint64_t)((unsigned __int128)M.r1 * M.r1 % q);
    M.r3 = (uint64_t)((unsigned __int128)M.r2 * M.r1 % q);
    return M;
}

}  // namespace lsr
