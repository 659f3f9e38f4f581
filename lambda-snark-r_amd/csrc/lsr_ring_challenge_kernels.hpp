// The fixed-point operator norm of ring elements and the rejection sampler of challenges built on it (batch.h "operator-norm-bounded
// ring challenges").
//
// N(c) = max over e in E of Re_e^2 + Im_e^2 with Re_e = sum_i c_i C[(i e) mod 2n], Im_e = sum_i c_i C[(i e - n/2) mod 2n] and the
// table C[j] = round(2^30 cos(pi j / n)) in LDS: integer sums of 32 x 32 + 64 multiply-adds, an unsigned 128-bit maximum.  The lanes
// split the points e; every lane walks the same terms (a broadcast read) and gathers its own two table entries per term.  The gather
// of term i has stride 2 i between neighbouring lanes: an odd i is conflict-free, i = 2^k m lands on 64 / 2^(k+1) banks but then only
// reads 2n / 2^(k+1) distinct words, half of them shared by lanes that a same-address read serves at once.
//   ring_opnorm_kernel: dense input, one workgroup per element (64 lanes at n <= 128, else 256).
//   ring_challenge_kernel: ONE WAVEFRONT owns an element and loops over its attempts, so the loop count is wave-uniform and the
//     loop holds no workgroup barrier (the waves of a workgroup only share the table, loaded once in front of the one barrier).  Per
//     attempt: the lanes produce the first-attempt stream blocks, lane 0 runs BALL's inside-out shuffle on 4-bit codes in LDS
//     (ball_draw of lsr_sampler.hpp at the attempt's word offset), the wave compacts the kappa non-zeros into 16-bit
//     (position, code) pairs, evaluates, reduces and compares.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "lsr_sampler.hpp"

namespace lsr {

constexpr int kOpnormMaxLog = 12;                        // n <= 4096: the table is 32 KiB
constexpr uint32_t kOpnormMaxCoefficient = 1u << 15;     // |c_i| <= 2^15: 2^12 2^15 2^30 = 2^57, every sum inside int64
constexpr uint32_t kChallengeAttemptWords = 1u << 18;    // LSR_RING_CHALLENGE_ATTEMPT_WORDS
constexpr uint32_t kChallengeMaxTries = 1024;            // LSR_RING_CHALLENGE_MAX_TRIES
constexpr uint32_t kChallengeChunkWords = 512;           // first-attempt words of a wave resident in LDS at a time: one block per lane
constexpr int kChallengeMaxWaves = 4;
constexpr uint32_t kChallengeLdsBytes = 64u << 10;

struct U128 {
    uint64_t lo, hi;
};
__device__ __forceinline__ bool u128_less(U128 a, U128 b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }

// re^2 + im^2 for |re|, |im| <= 2^57: below 2^115
__device__ __forceinline__ U128 opnorm_square_sum(int64_t re, int64_t im) {
    const uint64_t a = re < 0 ? 0 - (uint64_t)re : (uint64_t)re, b = im < 0 ? 0 - (uint64_t)im : (uint64_t)im;
    const uint64_t a_lo = a * a, b_lo = b * b;
    U128 r;
    r.lo = a_lo + b_lo;
    r.hi = __umul64hi(a, a) + __umul64hi(b, b) + (r.lo < a_lo ? 1u : 0u);
    return r;
}

// the maximum over the 64 lanes, in every lane (all lanes active)
__device__ __forceinline__ U128 opnorm_wave_max(U128 v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        U128 o;
        o.lo = __shfl_xor((unsigned long long)v.lo, s, 64);
        o.hi = __shfl_xor((unsigned long long)v.hi, s, 64);
        if (u128_less(v, o)) v = o;
    }
    return v;
}

// LDS written by some lanes of a wave and read by others of the same wave: DS operations of one wave execute in order, so only the
// compiler has to be held
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// max of Re_e^2 + Im_e^2 over the points k = first, first + stride, ... of E (negacyclic: e = 2k + 1, k < n/2; cyclic: e = 2k,
// k <= n/2).  terms.at(p, position, value) for p < count: coefficient `value` at X^position; every lane walks all of them.
template <class Terms>
__device__ __forceinline__ U128 opnorm_points(const int32_t* table, uint32_t logn, bool cyclic, const Terms terms, uint32_t count, uint32_t first,
                                              uint32_t stride) {
    const uint32_t n = 1u << logn, mask = 2 * n - 1, quarter = n >> 1;
    const uint32_t points = cyclic ? (n >> 1) + 1 : n >> 1;
    U128 best{0, 0};
    for (uint32_t k = first; k < points; k += stride) {
        const uint32_t e = cyclic ? 2 * k : 2 * k + 1;
        int64_t re = 0, im = 0;
        for (uint32_t p = 0; p < count; ++p) {
            uint32_t position;
            int32_t value;
            terms.at(p, position, value);
            const uint32_t a = (position * e) & mask;            // position < 2^12, e < 2^13
            re += (int64_t)value * table[a];
            im += (int64_t)value * table[(a - quarter) & mask];
        }
        const U128 s = opnorm_square_sum(re, im);
        if (u128_less(best, s)) best = s;
    }
    return best;
}

// ---- the stand-alone norm ------------------------------------------------------------------------------------------------------------
struct OpnormJob {
    uint64_t* out;            // [count][2]: low word, high word
    const uint64_t* x;        // [count][n]
    const int32_t* table;     // [2n]
    uint64_t count, q;
    uint32_t logn, cyclic;
};

struct DenseTerms {
    const int32_t* values;
    __device__ __forceinline__ void at(uint32_t p, uint32_t& position, int32_t& value) const {
        position = p;
        value = values[p];
    }
};

// dynamic LDS: 2n table words, then n centred coefficients (int32 each)
__global__ void __launch_bounds__(256) ring_opnorm_kernel(OpnormJob job) {
    extern __shared__ uint64_t opnorm_lds[];
    __shared__ U128 wave_best[4];
    const uint32_t n = 1u << job.logn, t = threadIdx.x, threads = blockDim.x;
    int32_t* const table = reinterpret_cast<int32_t*>(opnorm_lds);
    int32_t* const values = table + 2 * n;
    for (uint32_t x = t; x < 2 * n; x += threads) table[x] = job.table[x];
    const uint64_t half_q = job.q >> 1;
    for (uint64_t j = blockIdx.x; j < job.count; j += gridDim.x) {
        const uint64_t* e = job.x + (j << job.logn);
        __syncthreads();      // the table is there; the previous element's sums are done with `values` and thread 0 with wave_best
        int bad = 0;          // a word >= q, or a centred coefficient above 2^15 in magnitude
        for (uint32_t i = t; i < n; i += threads) {
            const uint64_t v = e[i];
            const bool high = v > half_q;
            const uint64_t magnitude = high ? job.q - v : v;
            const bool refuse = v >= job.q || magnitude > kOpnormMaxCoefficient;
            bad |= refuse;
            values[i] = refuse ? 0 : (high ? -(int32_t)magnitude : (int32_t)magnitude);
        }
        bad = __syncthreads_or(bad);      // (the barrier also publishes `values`)
        if (bad) {                        // the same in every lane of the workgroup
            if (t == 0) job.out[2 * j] = job.out[2 * j + 1] = ~0ull;
            continue;
        }
        const U128 best = opnorm_wave_max(opnorm_points(table, job.logn, job.cyclic != 0, DenseTerms{values}, n, t, threads));
        if ((t & 63u) == 0) wave_best[t >> 6] = best;
        __syncthreads();
        if (t == 0) {
            U128 all = best;
            for (uint32_t w = 1; w < threads / 64; ++w)
                if (u128_less(all, wave_best[w])) all = wave_best[w];
            job.out[2 * j] = all.lo;
            job.out[2 * j + 1] = all.hi;
        }
    }
}

// ---- the challenge sampler -----------------------------------------------------------------------------------------------------------
struct ChallengeJob {
    uint64_t* out;            // [count][n], element `first` at out
    int32_t* tries;           // [count], element `first` at tries
    const uint64_t* keys;     // as RingSampleJob
    const int32_t* table;     // [2n]; not read when check == 0
    uint64_t index_base, components, group_base, first, count, q;
    uint64_t bound_lo, bound_hi;      // T^2 2^60
    uint32_t kappa1, kappa2, max_tries;
    uint32_t check;           // 0: attempt 0 is taken
    uint32_t domain, logn, cyclic;
    uint32_t waves;           // elements in flight per workgroup: blockDim.x / 64
};

// The LDS of a workgroup: the table (check only), then per wave the first-attempt words of a chunk, the polynomial as 4-bit codes
// and (check only) the kappa pairs.  Every part is a multiple of 8 bytes.
struct ChallengeLayout {
    uint32_t table_bytes, chunk, codes_at, pairs_at, wave_bytes;
};
__host__ __device__ inline ChallengeLayout challenge_layout(uint32_t n, uint32_t kappa, bool check) {
    ChallengeLayout l;
    l.table_bytes = check ? 8 * n : 0;
    l.chunk = (kappa + 7u) & ~7u;
    if (l.chunk > kChallengeChunkWords) l.chunk = kChallengeChunkWords;
    l.codes_at = l.chunk * 8;
    l.pairs_at = l.codes_at + (((n + 7) / 8 * 4 + 7u) & ~7u);
    l.wave_bytes = l.pairs_at + (check ? (kappa * 2 + 7u) & ~7u : 0u);
    return l;
}

// the polynomial while the steps run: codes 0, 1 (+1), 2 (-1), 3 (+2), 4 (-2), eight to an LDS word
__device__ __forceinline__ uint32_t challenge_get(const uint32_t* codes, uint32_t i) { return (codes[i >> 3] >> ((i & 7u) * 4)) & 15u; }
__device__ __forceinline__ void challenge_set(uint32_t* codes, uint32_t i, uint32_t code) {
    const uint32_t shift = (i & 7u) * 4;
    codes[i >> 3] = (codes[i >> 3] & ~(15u << shift)) | (code << shift);
}
__device__ __forceinline__ int32_t challenge_code_value(uint32_t code) { return code == 0 ? 0 : (code == 1 ? 1 : (code == 2 ? -1 : (code == 3 ? 2 : -2))); }

// a non-zero coefficient: position in the low 12 bits, code above
struct PairTerms {
    const uint16_t* pairs;
    __device__ __forceinline__ void at(uint32_t p, uint32_t& position, int32_t& value) const {
        const uint32_t u = pairs[p];
        position = u & 4095u;
        value = challenge_code_value(u >> 12);
    }
};

// the candidate of attempt t into `codes` (the whole wave; complete and visible to every lane on return)
__device__ __forceinline__ void challenge_candidate(const ChallengeJob& job, const RingStream st, uint32_t t, uint32_t chunk, uint64_t* words,
                                                    uint32_t* codes, uint32_t lane) {
    const uint32_t n = 1u << job.logn, kappa = job.kappa1 + job.kappa2;
    const uint32_t base = t * kChallengeAttemptWords;
    for (uint32_t x = lane; x < (n + 7) / 8; x += 64) codes[x] = 0;
    for (uint32_t s0 = 0; s0 < kappa; s0 += chunk) {
        const uint32_t now = min(chunk, kappa - s0);
        wave_lds_sync();                                     // lane 0 is done with the previous chunk's words
        if (lane * 8 < now) {                                // chunk <= 512: one block per lane
            uint64_t w[8];
            stream_block(st.key, job.domain, st.index, ((base + s0) >> 3) + lane, w);      // base and s0 are multiples of 8
#pragma unroll
            for (int k = 0; k < 8; ++k) words[lane * 8 + k] = w[k];                        // (lane * 8 + k < chunk: a multiple of 8)
        }
        wave_lds_sync();
        if (lane == 0) {
            for (uint32_t s = s0; s < s0 + now; ++s) {
                const uint64_t word = words[s - s0];
                const uint32_t i = n - kappa + s;
                const uint32_t j = i == 0 ? 0u : ball_draw(st, job.domain, kappa, s, i, word, base);
                challenge_set(codes, i, challenge_get(codes, j));
                challenge_set(codes, j, (s < job.kappa2 ? 3u : 1u) + (uint32_t)(word >> 63));
            }
        }
    }
    wave_lds_sync();
}

// dynamic LDS: challenge_layout(n, kappa, check): table_bytes + waves * wave_bytes
__global__ void __launch_bounds__(64 * kChallengeMaxWaves) ring_challenge_kernel(ChallengeJob job) {
    extern __shared__ uint64_t challenge_lds[];
    const uint32_t n = 1u << job.logn, kappa = job.kappa1 + job.kappa2;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const ChallengeLayout lay = challenge_layout(n, kappa, job.check != 0);
    int32_t* const table = reinterpret_cast<int32_t*>(challenge_lds);
    unsigned char* const mine = reinterpret_cast<unsigned char*>(challenge_lds) + lay.table_bytes + wave * lay.wave_bytes;
    uint64_t* const words = reinterpret_cast<uint64_t*>(mine);
    uint32_t* const codes = reinterpret_cast<uint32_t*>(mine + lay.codes_at);
    uint16_t* const pairs = reinterpret_cast<uint16_t*>(mine + lay.pairs_at);
    if (job.check)
        for (uint32_t x = threadIdx.x; x < 2 * n; x += blockDim.x) table[x] = job.table[x];
    __syncthreads();          // the workgroup's only barrier: from here on every wave runs alone
    const U128 bound{job.bound_lo, job.bound_hi};
    for (uint64_t local = (uint64_t)blockIdx.x * job.waves + wave; local < job.count; local += (uint64_t)gridDim.x * job.waves) {
        const RingStream st = ring_stream_of(job.keys, job.first + local, job.components, job.group_base, job.index_base);
        uint32_t taken = 0;   // attempts used, 0: none passed
        for (uint32_t t = 0; t < job.max_tries && !taken; ++t) {
            challenge_candidate(job, st, t, lay.chunk, words, codes, lane);
            if (!job.check) {
                taken = 1;
                break;
            }
            uint32_t found = 0;
            for (uint32_t x0 = 0; x0 < n; x0 += 64) {
                const uint32_t x = x0 + lane;
                const uint32_t code = x < n ? challenge_get(codes, x) : 0u;
                const unsigned long long set = __ballot(code != 0);
                const uint32_t at = found + __popcll(set & ((1ull << lane) - 1));
                if (code && at < kappa) pairs[at] = (uint16_t)(x | (code << 12));      // (a shuffle of kappa steps leaves kappa non-zeros)
                found += __popcll(set);
            }
            wave_lds_sync();
            const U128 norm = opnorm_wave_max(opnorm_points(table, job.logn, job.cyclic != 0, PairTerms{pairs}, kappa, lane, 64));
            // (the same in every lane: the scalar makes the branch wave-uniform for the compiler too)
            if (__builtin_amdgcn_readfirstlane(u128_less(bound, norm) ? 0 : 1)) taken = t + 1;
        }
        uint64_t* const dst = job.out + (local << job.logn);
        for (uint32_t x = lane; x < n; x += 64) {
            const uint32_t code = taken ? challenge_get(codes, x) : 0u;
            const uint64_t magnitude = code >= 3 ? 2 : 1;
            dst[x] = code == 0 ? 0 : ((code & 1u) ? magnitude : job.q - magnitude);
        }
        if (lane == 0) job.tries[local] = (int32_t)taken;
        wave_lds_sync();      // the codes are cleared for the wave's next element
    }
}

}  // namespace lsr
