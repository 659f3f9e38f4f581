// Norms and projections of ring vectors (batch.h "norms and projections of ring vectors"): the exact l2 norm squared
// as a 128-bit integer, the Johnson-Lindenstrauss projection p = Pi s with Pi generated from the ChaCha20 streams of lsr_sampler.hpp
// while it is applied, and the rows of Pi as ring elements.  Integer code that reads only q and n of a context.
//
// A vector is `width` ring elements, len = width n canonical words; position pos = c n + k.  Entry pi[r][pos] is the 2-bit field
// f = (word[pos / 32] >> 2 (pos % 32)) & 3 of the row's stream, (f & 1) - (f >> 1): one stream block is 256 entries.
//   PROJECT: one lane owns one row r, a workgroup of 256 lanes covers the 256 rows over a slice of kProjectSlice positions of one
//     vector.  A lane generates the blocks of its own row for the slice and accumulates in two registers; the coefficient at a
//     position is the same in every lane, so there is no cross-lane step at all.  Slices are combined by 64-bit integer atomics into
//     an output that ring_project_init_kernel zeroed (wrapping adds of exact int64 terms: any order gives the same word), the status
//     by an atomic minimum (1 done > 0 over the bound > -1 a word >= q), and ring_project_finish_kernel clears the outputs of a
//     vector whose status is not 1.  Three launches, nothing allocated.
//   L2SQ: one workgroup per vector, a 128-bit sum per lane with a sticky overflow bit (the terms are non-negative, so a partial sum
//     that overflows means the total does: the saturation does not depend on the order), wave reduction, the waves through LDS.
//   MATRIX: a workgroup generates 256 blocks of one row into LDS (one block per lane) and writes the 65536 entries coalesced.
//   ADJOINT (§5k): out = Pi^T w.  A workgroup generates one block of all 256 rows into LDS (one row per lane); then a lane owns one
//     position and walks the rows with the weights broadcast from LDS.  One launch that writes every output word and the status.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "lsr_sampler.hpp"

namespace lsr {

constexpr int kProjectRows = 256;                 // LSR_RING_PROJECT_ROWS: one lane per row
constexpr uint32_t kProjectSlice = 2048;          // positions per workgroup: eight stream blocks per lane
constexpr int kNormThreads = 256;

struct ProjectJob {
    int64_t* out;             // [count][256], vector `first` of the call at out
    int32_t* status;          // [count]
    const uint64_t* x;        // [count][len]
    const uint64_t* keys;     // [groups][4]: the key of vector j is keys[4 (j / components - group_base) ..]
    uint64_t index_base;      // row r of vector j is stream index index_base + 256 (j % components) + r
    uint64_t components;
    uint64_t group_base;      // the first key group present at `keys` (host staging uploads the groups of one chunk)
    uint64_t first;           // vectors [first, first + gridDim.x / slices) of the call
    uint64_t len;             // width n, at most 2^32
    uint64_t q, bound;
    uint32_t slices;          // ceil(len / kProjectSlice)
    uint32_t domain;
};

__global__ void __launch_bounds__(kNormThreads) ring_project_init_kernel(int64_t* __restrict__ out, int32_t* __restrict__ status, size_t count) {
    const size_t total = count * kProjectRows;
    for (size_t i = (size_t)blockIdx.x * kNormThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kNormThreads) {
        out[i] = 0;
        if ((i & (kProjectRows - 1)) == 0) status[i / kProjectRows] = 1;
    }
}

__global__ void __launch_bounds__(kNormThreads) ring_project_finish_kernel(int64_t* __restrict__ out, const int32_t* __restrict__ status, size_t count) {
    for (size_t j = blockIdx.x; j < count; j += gridDim.x)
        if (status[j] != 1) out[j * kProjectRows + threadIdx.x] = 0;
}

// plus - minus += pi * c for the 16 entries of one 32-bit half of a stream word; c: their centred coefficients (LDS, the same address
// in every lane: a broadcast)
__device__ __forceinline__ void project_half_word(uint32_t half, uint64_t& plus, uint64_t& minus, const int64_t* c) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const uint64_t v = (uint64_t)c[e];
        const uint64_t take = 0ull - (uint64_t)((half >> (2 * e)) & 1u);          // f & 1: +c
        const uint64_t drop = 0ull - (uint64_t)((half >> (2 * e + 1)) & 1u);      // f >> 1: -c
        plus += v & take;
        minus += v & drop;
    }
}

__global__ void __launch_bounds__(kNormThreads) ring_project_kernel(ProjectJob job) {
    __shared__ int64_t staged[kProjectSlice];
    const uint32_t r = threadIdx.x;
    const uint64_t local = blockIdx.x / job.slices;
    const uint32_t slice = blockIdx.x - (uint32_t)(local * job.slices);
    const uint64_t p0 = (uint64_t)slice * kProjectSlice;
    const uint32_t now = (uint32_t)min((uint64_t)kProjectSlice, job.len - p0);
    const uint64_t* __restrict__ xs = job.x + local * job.len + p0;
    const uint64_t q = job.q, half_q = job.q >> 1, bound = job.bound;
    const RingStream st = ring_stream_of(job.keys, job.first + local, job.components, job.group_base, 0);      // index: j % components
    const uint64_t index = job.index_base + (uint64_t)kProjectRows * st.index + r;
    const uint32_t block0 = (uint32_t)(p0 >> 8);      // kProjectSlice is a multiple of 256
    uint64_t plus = 0, minus = 0;

    // Every lane tests eight words of the slice and stages them centred: the status rides on the one read of x.  (The other way to
    // read a wavefront-uniform coefficient, scalar loads with the centring on the scalar unit, measured about 2.5 % slower:
    // DESIGN.md §5i, tools/experiments/ring_project_scalar_loads.hpp.txt.)
    bool not_below_q = false, over_bound = false;
    for (uint32_t i = r; i < kProjectSlice; i += kNormThreads) {      // (positions behind the vector's end read as 0)
        const uint64_t v = i < now ? xs[i] : 0;
        const bool high = v > half_q;
        not_below_q |= v >= q;
        over_bound |= (high ? q - v : v) > bound;
        staged[i] = (int64_t)(high ? v - q : v);
    }
    not_below_q = __syncthreads_or(not_below_q);      // (the barrier also publishes `staged`)
    over_bound = __syncthreads_or(over_bound);
    if (not_below_q || over_bound) {                  // the same in every lane of the workgroup
        if (r == 0) atomicMin(job.status + local, not_below_q ? -1 : 0);
        return;
    }

    // The sums, one stream block (256 entries) at a time: the staged slice read back as broadcasts (zero behind the vector's end, so
    // every block is whole).
    for (uint32_t b = 0; b * 256 < now; ++b) {
        uint64_t w[8];
        stream_block(st.key, job.domain, index, block0 + b, w);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int64_t* at = staged + b * 256 + t * 32;
            project_half_word((uint32_t)w[t], plus, minus, at);
            project_half_word((uint32_t)(w[t] >> 32), plus, minus, at + 16);
        }
    }
    atomicAdd(reinterpret_cast<unsigned long long*>(job.out + local * kProjectRows + r), (unsigned long long)(plus - minus));
}

// out[j] = {low, high} of sum centred^2 over the len words of vector j, or all ones (a word >= q, or a sum of 2^128 - 1 or more)
__global__ void __launch_bounds__(kNormThreads) ring_l2sq_kernel(uint64_t* __restrict__ out, const uint64_t* __restrict__ x, size_t count, uint64_t len,
                                                                 uint64_t q) {
    __shared__ uint64_t wave_lo[kNormThreads / 64], wave_hi[kNormThreads / 64];
    __shared__ uint32_t wave_bad[kNormThreads / 64];
    const uint64_t half_q = q >> 1;
    const uint32_t t = threadIdx.x;
    for (size_t j = blockIdx.x; j < count; j += gridDim.x) {
        const uint64_t* e = x + j * len;
        uint64_t lo = 0, hi = 0;
        uint32_t bad = 0;      // a word >= q, or a carry out of bit 127
#pragma unroll 4
        for (uint64_t k = t; k < len; k += kNormThreads) {
            const uint64_t v = e[k];
            const uint64_t a = v > half_q ? q - v : v;
            bad |= v >= q;
            const uint64_t sq_lo = a * a, sq_hi = __umul64hi(a, a);
            lo += sq_lo;
            const uint64_t carry = lo < sq_lo;
            hi += sq_hi;
            bad |= hi < sq_hi;
            hi += carry;
            bad |= hi < carry;
        }
        auto add = [&](uint64_t o_lo, uint64_t o_hi, uint32_t o_bad) {
            lo += o_lo;
            const uint64_t carry = lo < o_lo;
            hi += o_hi;
            bad |= o_bad | (hi < o_hi);
            hi += carry;
            bad |= hi < carry;
        };
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            const uint64_t o_lo = __shfl_xor((unsigned long long)lo, s, 64), o_hi = __shfl_xor((unsigned long long)hi, s, 64);
            const uint32_t o_bad = __shfl_xor(bad, s, 64);
            add(o_lo, o_hi, o_bad);
        }
        if ((t & 63u) == 0) {
            wave_lo[t >> 6] = lo;
            wave_hi[t >> 6] = hi;
            wave_bad[t >> 6] = bad;
        }
        __syncthreads();
        if (t == 0) {
            for (uint32_t w = 1; w < kNormThreads / 64; ++w) add(wave_lo[w], wave_hi[w], wave_bad[w]);
            const bool saturated = bad || (lo == ~0ull && hi == ~0ull);
            out[2 * j] = saturated ? ~0ull : lo;
            out[2 * j + 1] = saturated ? ~0ull : hi;
        }
        __syncthreads();      // the wave slots are written again for the workgroup's next vector
    }
}

struct ProjectMatrixJob {
    uint64_t* out;            // [rows][len]
    const uint64_t* key;      // four words
    uint64_t index;           // stream index of the first row written: index_base + rows_first
    uint64_t len, q;
    uint32_t chunks;          // ceil(len / 65536): workgroups per row
    uint32_t domain;
};

// workgroup (row, chunk): lane l generates block 256 chunk + l of the row's stream into LDS; then entry 256 i + l of the chunk is
// written by lane l for i = 0 .. 255 — consecutive lanes, consecutive words
__global__ void __launch_bounds__(kNormThreads) ring_project_matrix_kernel(ProjectMatrixJob job) {
    __shared__ uint64_t words[kNormThreads * 8];
    const uint32_t row = blockIdx.x / job.chunks, chunk = blockIdx.x - row * job.chunks, l = threadIdx.x;
    const uint64_t p0 = (uint64_t)chunk << 16;
    const uint32_t now = (uint32_t)min((uint64_t)1 << 16, job.len - p0);
    if ((uint64_t)l * 256 < now) {
        uint64_t w[8];
        stream_block(job.key, job.domain, job.index + row, chunk * 256 + l, w);
#pragma unroll
        for (int t = 0; t < 8; ++t) words[l * 8 + t] = w[t];
    }
    __syncthreads();
    uint64_t* dst = job.out + (uint64_t)row * job.len + p0;
    for (uint32_t i = l; i < now; i += kNormThreads) {
        const uint32_t f = (uint32_t)(words[i >> 5] >> (2 * (i & 31u))) & 3u;
        dst[i] = f == 1 ? 1 : (f == 2 ? job.q - 1 : 0);
    }
}

// ---- the adjoint Pi^T w --------------------------------------------------------------------------------------------------
// The dual of PROJECT: there a lane owns a row and the coefficient is broadcast, here a lane owns a position and the weight is.

#ifndef LSR_ADJOINT_SET_BLOCK
#define LSR_ADJOINT_SET_BLOCK 4                   // weight sets accumulated per pass over the rows (1, 2 or 4; timed in §5k)
#endif
constexpr int kAdjointSetBlock = LSR_ADJOINT_SET_BLOCK;
constexpr int kAdjointMaxSets = 16;               // LSR_RING_PROJECT_ADJOINT_MAX_SETS
constexpr int kAdjointRowPitch = kProjectRows + 8;      // dwords between half-word h and h + 1 of the rows: four consecutive h, four banks
static_assert(kAdjointSetBlock == 1 || kAdjointSetBlock == 2 || kAdjointSetBlock == 4, "the set block is 1, 2 or 4");

struct ProjectAdjointJob {
    uint64_t* out;            // [count][sets][len], vector `first` of the call at out
    int32_t* status;          // [count]
    const uint64_t* weights;  // [groups][sets][256], the group of vector j at weights + (j / components - group_base) sets 256
    const uint64_t* keys;     // [groups][4], as ProjectJob
    uint64_t index_base;
    uint64_t components;
    uint64_t group_base;
    uint64_t first;           // vectors [first, first + gridDim.x / blocks) of the call
    uint64_t len;             // width n, at most 2^32
    uint64_t n;               // a power of two
    uint64_t q;
    uint32_t blocks;          // ceil(len / 256): workgroups per vector
    uint32_t sets;
    uint32_t domain;
    uint32_t conjugate;       // 0: as computed; 1: X -> X^(n-1) of X^n - 1; 2: X -> X^(2n-1) of X^n + 1
};

// LIVE sets over the 256 rows for the position whose 2-bit field sits at bit `shift` of the half-words halves[r] (consecutive rows,
// consecutive dwords: a wavefront reads four addresses in four banks).  wt: [kAdjointSetBlock][256] weights (the same address in every
// lane: a broadcast), WIDE: followed by their negatives mod q.  Not WIDE (q < 2^55): two plain sums of at most 256 words below 2^55
// and one reduction of their difference.  WIDE: one sum mod q, a conditional subtraction per step that also covers the carry out of
// bit 63 (q up to 2^64).
template <int LIVE, bool WIDE>
__device__ __forceinline__ void adjoint_rows(const uint32_t* halves, uint32_t shift, const uint64_t* wt, uint64_t q, uint64_t (&res)[kAdjointSetBlock]) {
    if constexpr (WIDE) {
        uint64_t acc[LIVE];
#pragma unroll
        for (int k = 0; k < LIVE; ++k) acc[k] = 0;
#pragma unroll 4
        for (int r = 0; r < kProjectRows; ++r) {
            const uint32_t f =(halves[r] >> shift) & 3u;
            const uint64_t take = 0ull - (uint64_t)(f == 1u), drop = 0ull - (uint64_t)(f == 2u);
#pragma unroll
            for (int k = 0; k < LIVE; ++k) {
                const uint64_t v = (wt[k * kProjectRows + r] & take) | (wt[(kAdjointSetBlock + k) * kProjectRows + r] & drop);
                const uint64_t t = acc[k] + v;                       // acc, v < q: the true sum is below 2 q
                acc[k] = (t < v || t >= q) ? t - q : t;
            }
        }
#pragma unroll
        for (int k = 0; k < LIVE; ++k) res[k] = acc[k];
    } else {
        uint64_t plus[LIVE], minus[LIVE];
#pragma unroll
        for (int k = 0; k < LIVE; ++k) plus[k] = minus[k] = 0;
#pragma unroll 8
        for (int r = 0; r < kProjectRows; ++r) {
            // the field's two bits moved to bit 31 and spread by an arithmetic shift: one 32-bit mask serves both halves of a word
            const uint32_t h = halves[r];
            const uint64_t take = (uint64_t)(int64_t)((int32_t)(h << (31u - shift)) >> 31);                 // f & 1: +w
            const uint64_t drop = (uint64_t)(int64_t)((int32_t)(h << (30u - shift)) >> 31);                 // f >> 1: -w; f = 3: both, 0
#pragma unroll
            for (int k = 0; k < LIVE; ++k) {
                const uint64_t w = wt[k * kProjectRows + r];
                plus[k] += w & take;
                minus[k] += w & drop;
            }
        }
#pragma unroll
        for (int k = 0; k < LIVE; ++k) {
            const int64_t d = (int64_t)(plus[k] - minus[k]);         // both below 2^63: the difference is exact
            const uint64_t m = (uint64_t)(d < 0 ? -d : d) % q;
            res[k] = (d < 0 && m != 0) ? q - m : m;
        }
    }
}

// workgroup (vector, block): positions [256 block, 256 block + 256) of one vector for every set.  Lane r generates block `block` of
// row r once; then lane p owns position 256 block + p.  The kernel writes every output word and the status itself.
template <bool WIDE>
__global__ void __launch_bounds__(kNormThreads) ring_project_adjoint_kernel(ProjectAdjointJob job) {
    __shared__ uint32_t halves[16 * kAdjointRowPitch];                                 // half-word h of row r at h pitch + r
    __shared__ uint64_t wt[(WIDE ? 2 : 1) * kAdjointSetBlock * kProjectRows];
    const uint32_t t = threadIdx.x;
    const uint32_t local = blockIdx.x / job.blocks, block = blockIdx.x - local * job.blocks;
    const uint64_t q = job.q;
    const RingStream st = ring_stream_of(job.keys, job.first + local, job.components, job.group_base, 0);      // index: j % components
    const uint64_t* __restrict__ wg = job.weights + (uint64_t)((st.key - job.keys) >> 2) * job.sets * kProjectRows;
    {
        uint64_t w[8];
        stream_block(st.key, job.domain, job.index_base + (uint64_t)kProjectRows * st.index + t, block, w);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            halves[(2 * i) * kAdjointRowPitch + t] = (uint32_t)w[i];
            halves[(2 * i + 1) * kAdjointRowPitch + t] = (uint32_t)(w[i] >> 32);
        }
    }
    bool not_below_q = false;
    for (uint32_t k = 0; k < job.sets; ++k) not_below_q |= wg[k * kProjectRows + t] >= q;
    not_below_q = __syncthreads_or(not_below_q);      // (the barrier also publishes `halves`)
    if (block == 0 && t == 0) job.status[local] = not_below_q ? -1 : 1;

    // position and destination of this lane: element base + i -> base + (n - i) mod n under the conjugation, negated in X^n + 1
    const uint64_t pos = (uint64_t)block * 256 + t;
    const bool live = pos < job.len;
    const uint64_t i = pos & (job.n - 1);
    const uint64_t dest = job.conjugate ? pos - i + ((job.n - i) & (job.n - 1)) : pos;
    const bool negate = job.conjugate == 2 && i != 0;
    uint64_t* __restrict__ o = job.out + (uint64_t)local * job.sets * job.len + dest;
    if (not_below_q) {                                // the same in every lane of the workgroup
        if (live)
            for (uint32_t k = 0; k < job.sets; ++k) o[k * job.len] = 0;
        return;
    }
    const uint32_t* mine = halves + (t >> 4) * kAdjointRowPitch;
    const uint32_t shift = 2 * (t & 15u);
    for (uint32_t k0 = 0; k0 < job.sets; k0 += kAdjointSetBlock) {
        const uint32_t now = min((uint32_t)kAdjointSetBlock, job.sets - k0);
        if (k0) __syncthreads();                      // the previous block of sets has been read
        for (uint32_t k = 0; k < now; ++k) {
            const uint64_t w = wg[(k0 + k) * kProjectRows + t];
            wt[k * kProjectRows + t] = w;
            if constexpr (WIDE) wt[(kAdjointSetBlock + k) * kProjectRows + t] = w ? q - w : 0;
        }
        __syncthreads();
        uint64_t res[kAdjointSetBlock];
        switch (now) {                                // the same in every lane
            case 1: adjoint_rows<1, WIDE>(mine, shift, wt, q, res); break;
            case 2: if constexpr (kAdjointSetBlock >= 2) adjoint_rows<2, WIDE>(mine, shift, wt, q, res); break;
            case 3: if constexpr (kAdjointSetBlock >= 4) adjoint_rows<3, WIDE>(mine, shift, wt, q, res); break;
            default: if constexpr (kAdjointSetBlock >= 4) adjoint_rows<4, WIDE>(mine, shift, wt, q, res); break;
        }
#pragma unroll
        for (uint32_t k = 0; k < (uint32_t)kAdjointSetBlock; ++k)      // (unrolled: res stays in registers)
            if (live && k < now) o[(uint64_t)(k0 + k) * job.len] = (negate && res[k] != 0) ? q - res[k] : res[k];
    }
}

}  // namespace lsr
