// Exact sampling of ring elements from the ChaCha20 streams of lsr_sampler.hpp (batch.h "seeded ring sampling").
//
// draw(m; w_0, w_1, ...; U): L = bitlen(m - 1), F = floor(U / L); the candidates of a word are its F low L-bit fields, scanned in
// order; the first candidate below m is the result; after kRingSampleMaxWords words field 0 of the last word is reduced mod m.
//   UNIFORM / BOUNDED: coefficient i of an element draws from the words a n + i (a = 0, 1, ...), U = 64.  One lane = one stream
//     block = eight coefficients (n >= 8): attempt a of all eight sits in ONE block, a (n/8) + k, at the coefficients' own slots.
//     The fast path is one compare per word and eight unconditional stores; a lane with a rejected coefficient goes on in
//     ring_sample_refill and overwrites only what is missing.  (Inlined: a call would pass the words through the stack, and no
//     kernel here uses scratch.)  n < 8: one lane = one element (ring_sample_small_kernel).
//   BALL: one workgroup per element; the polynomial as 2-bit codes in LDS (n <= 131072) or as its final words in the output itself
//     (large cyclic contexts); the first-attempt words in LDS, computed by all lanes; the kappa dependent steps in lane 0.
// Nothing here is constant-time, and nothing needs to be: a rejected candidate is a field of the stream that no accepted value
// depends on.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "lsr_sampler.hpp"

namespace lsr {

constexpr int kRingSampleThreads = 256;
constexpr uint32_t kBallChunkWords = 2048;          // first-attempt words resident in LDS at a time: one block per lane
constexpr int kBallLdsMaxLog = 17;                  // the polynomial as 2-bit codes: 32 KiB at n = 131072

struct RingSampleJob {
    uint64_t* out;            // [count][n], element `first` at out
    const uint64_t* keys;     // [groups][4]: the key of element e is keys[4 (e / components - group_base) ..]
    uint64_t index_base;      // stream index of element e = index_base + e % components
    uint64_t components;
    uint64_t group_base;      // the first key group present at `keys` (host staging uploads the groups of one chunk)
    uint64_t first, count;    // elements [first, first + count) of the call
    uint64_t q;
    uint64_t m;               // UNIFORM: q; BOUNDED: 2 beta + 1
    uint64_t beta;            // UNIFORM: 0
    uint64_t mask;            // 2^L - 1, L = bitlen(m - 1) (all ones at L = 64: never a shift by 64)
    uint32_t width;           // L
    uint32_t fields;          // F = 64 / L
    uint32_t domain;
    uint32_t logn;
};

// (RingStream and ring_stream_of, the key and stream index of element e: lsr_sampler.hpp)

// r in [0, m) -> the stored word: r - beta as a canonical residue (beta = 0: r itself)
__device__ __forceinline__ uint64_t ring_sample_value(uint64_t r, uint64_t beta, uint64_t q) { return r >= beta ? r - beta : q - (beta - r); }

// (ring_sample_last_resort, ring_sample_scan and ball_draw, shared with lsr_ring_challenge_kernels.hpp: lsr_sampler.hpp)

// The slow path of a lane: `pending` (bit s: coefficient s of the block has no value yet) after field 0 of the first-attempt words
// w; fills only what is missing.
__device__ __forceinline__ void ring_sample_refill(const RingSampleJob& job, const RingStream st, uint32_t block, uint32_t blocks_per_attempt,
                                                uint64_t (&w)[8], uint32_t pending, uint64_t* dst) {
    uint64_t r;
#pragma unroll
    for (int s = 0; s < 8; ++s)
        if ((pending >> s & 1u) && ring_sample_scan(w[s], 1, job.fields, job.width, job.mask, job.m, r)) {
            dst[s] = ring_sample_value(r, job.beta, job.q);
            pending &= ~(1u << s);
        }
    for (uint32_t a = 1; a < kRingSampleMaxWords && pending; ++a) {
        stream_block(st.key, job.domain, st.index, a * blocks_per_attempt + block, w);
#pragma unroll
        for (int s = 0; s < 8; ++s)
            if ((pending >> s & 1u) && ring_sample_scan(w[s], 0, job.fields, job.width, job.mask, job.m, r)) {
                dst[s] = ring_sample_value(r, job.beta, job.q);
                pending &= ~(1u << s);
            }
    }
#pragma unroll
    for (int s = 0; s < 8; ++s)
        if (pending >> s & 1u) dst[s] = ring_sample_value(ring_sample_last_resort(w[s], job.mask, job.m), job.beta, job.q);
}

// n >= 8.  gid -> (element, block) by a shift: ring degrees are powers of two.
__global__ void __launch_bounds__(kRingSampleThreads) ring_sample_kernel(RingSampleJob job) {
    const uint32_t block_log = job.logn - 3;
    const uint64_t gid = (uint64_t)blockIdx.x * kRingSampleThreads + threadIdx.x;
    const uint64_t local = gid >> block_log;
    if (local >= job.count) return;
    const uint32_t block = (uint32_t)(gid & ((1ull << block_log) - 1));
    const RingStream st = ring_stream_of(job.keys, job.first + local, job.components, job.group_base, job.index_base);
    uint64_t w[8];
    stream_block(st.key, job.domain, st.index, block, w);
    uint64_t* dst = job.out + (gid << 3);
    uint32_t pending = 0;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const uint64_t c = w[s] & job.mask;
        dst[s] = ring_sample_value(c, job.beta, job.q);      // (a rejected slot is overwritten by this lane below)
        pending |= (c < job.m ? 0u : 1u) << s;
    }
    if (pending) ring_sample_refill(job, st, block, 1u << block_log, w, pending, dst);
}

// n = 2 or 4: one lane = one element.  Word x of the stream is attempt x / n of coefficient x % n, so a scan of the words in order
// meets the attempts of every coefficient in order; 64 n words = 8 n blocks at the most.
__global__ void __launch_bounds__(kRingSampleThreads) ring_sample_small_kernel(RingSampleJob job) {
    const uint64_t local = (uint64_t)blockIdx.x * kRingSampleThreads + threadIdx.x;
    if (local >= job.count) return;
    const uint32_t n = 1u << job.logn;
    const RingStream st = ring_stream_of(job.keys, job.first + local, job.components, job.group_base, job.index_base);
    uint64_t* dst = job.out + (local << job.logn);
    uint32_t pending = (1u << n) - 1;
    uint64_t w[8];
    for (uint32_t block = 0; block < 8 * n && pending; ++block) {
        stream_block(st.key, job.domain, st.index, block, w);
        const bool last = block >= 8 * n - (n + 7) / 8;      // the blocks that hold attempt 63 (8 is a multiple of n: one block)
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const uint32_t i = (uint32_t)s & (n - 1);        // (8 block + s) % n
            if (!(pending >> i & 1u)) continue;
            uint64_t r;
            bool done = ring_sample_scan(w[s], 0, job.fields, job.width, job.mask, job.m, r);
            if (!done && last && (uint32_t)s >= 8 - n) {     // attempt 63 of coefficient i
                r = ring_sample_last_resort(w[s], job.mask, job.m);
                done = true;
            }
            if (done) {
                dst[i] = ring_sample_value(r, job.beta, job.q);
                pending &= ~(1u << i);
            }
        }
    }
}

// ---- BALL -----------------------------------------------------------------------------------------------------------------------
struct RingBallJob {
    uint64_t* out;
    const uint64_t* keys;
    uint64_t index_base, components, group_base, first, count, q;
    uint32_t kappa, domain, logn;
};

// the polynomial while the steps run: codes 0, 1 (+1), 2 (-1), sixteen to an LDS word — or the final words in the output (LDS = false)
template <bool LDS>
__device__ __forceinline__ uint32_t ball_get(const uint32_t* codes, const uint64_t* dst, uint32_t i) {
    if constexpr (LDS) return (codes[i >> 4] >> ((i & 15u) * 2)) & 3u;
    const uint64_t v = dst[i];
    return v == 0 ? 0u : (v == 1 ? 1u : 2u);
}
template <bool LDS>
__device__ __forceinline__ void ball_set(uint32_t* codes, uint64_t* dst, uint32_t i, uint32_t code, uint64_t q) {
    if constexpr (LDS) {
        const uint32_t shift = (i & 15u) * 2;
        codes[i >> 4] = (codes[i >> 4] & ~(3u << shift)) | (code << shift);
    } else {
        dst[i] = code == 0 ? 0 : (code == 1 ? 1 : q - 1);
    }
}

// dynamic LDS: min(kappa rounded up to 8, kBallChunkWords) words, then (LDS) n / 16 code words (at least one)
template <bool LDS>
__global__ void __launch_bounds__(kRingSampleThreads) ring_sample_ball_kernel(RingBallJob job) {
    extern __shared__ uint64_t ball_lds[];
    const uint32_t n = 1u << job.logn, kappa = job.kappa;
    const uint32_t chunk = min((kappa + 7u) & ~7u, kBallChunkWords);
    uint64_t* const words = ball_lds;
    uint32_t* const codes = reinterpret_cast<uint32_t*>(ball_lds + chunk);
    for (uint64_t local = blockIdx.x; local < job.count; local += gridDim.x) {
        const RingStream st = ring_stream_of(job.keys, job.first + local, job.components, job.group_base, job.index_base);
        uint64_t* const dst = job.out + (local << job.logn);
        if constexpr (LDS) {
            for (uint32_t x = threadIdx.x; x < (n + 15) / 16; x += kRingSampleThreads) codes[x] = 0;
        } else {
            for (uint32_t x = threadIdx.x; x < n; x += kRingSampleThreads) dst[x] = 0;
        }
        for (uint32_t s0 = 0; s0 < kappa; s0 += chunk) {
            const uint32_t now = min(chunk, kappa - s0);
            __syncthreads();                                 // the previous chunk's steps (or element's stores) are done with `words`
            for (uint32_t b = threadIdx.x; b * 8 < now; b += kRingSampleThreads) {
                uint64_t w[8];
                stream_block(st.key, job.domain, st.index, (s0 >> 3) + b, w);      // s0 is a multiple of 8
#pragma unroll
                for (int t = 0; t < 8; ++t) words[b * 8 + t] = w[t];               // (b * 8 + t < chunk: chunk is a multiple of 8)
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                for (uint32_t s = s0; s < s0 + now; ++s) {
                    const uint64_t word = words[s - s0];
                    const uint32_t i = n - kappa + s;
                    const uint32_t j = i == 0 ? 0u : ball_draw(st, job.domain, kappa, s, i, word);
                    ball_set<LDS>(codes, dst, i, ball_get<LDS>(codes, dst, j), job.q);
                    ball_set<LDS>(codes, dst, j, (word >> 63) ? 2u : 1u, job.q);
                }
            }
        }
        if constexpr (LDS) {
            __syncthreads();
            for (uint32_t x = threadIdx.x; x < n; x += kRingSampleThreads) {
                const uint32_t code = ball_get<true>(codes, dst, x);
                dst[x] = code == 0 ? 0 : (code == 1 ? 1 : job.q - 1);
            }
        }
        __syncthreads();
    }
}

}  // namespace lsr
