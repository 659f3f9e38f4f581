// Batched linear combination of device-resident commitment rows (lsr_lwe_combine_rows_device):
//     out_j = sum_{i < terms} c'_{j,i} * row[j * term_stride + i]        over the body residues, each under its own modulus,
// c'_{j,i} = the centred representative of coeffs[j][i] mod t — lwe_linear_combine (commitment.cpp:247-266) for a whole batch.
//
// Two launches, no workspace:
//   combine_prologue_kernel   one workgroup per output: header screening of its term rows, the exact integer weight sum |c'| against the
//                             host-computed budget, status = 1 / 0 / -1, and the output row's header
//   combine_body_kernel       a skinny modular GEMM: a workgroup owns 256 body words x kCombineOutputs outputs (one word and
//                             kCombineOutputs accumulators per lane).  Terms are consumed kCombineTerms at a time: the 256 lanes reduce
//                             the 256 coefficients of the step (one each) into LDS, every lane then reads them back at wave-uniform
//                             addresses.  SHARED (term_stride == 0): a term word is loaded once and feeds every output of the tile.
//                             A body residue >= its modulus lowers the status of the outputs it feeds to -1.
// FP64 flavour (q < 2^45; default and RNS contexts): mulmod_f64(word, c') with the SIGNED small integer c' (|c'| <= t/2 < 2^20) — the
// same multiplier under both primes of an RNS row — products accumulated unreduced, canonical_f64 every kCombineTerms terms:
//     |acc| <= q + kCombineTerms * 0.875 q = 29 q <= 32 q, the bound of canonical_f64 (lsr_arith.hpp); every partial sum is an
//     exact integer below 2^50.
// u64 flavour (wide contexts, or lsr_set_arith_mode): mulmod_barrett128 with the residue q - |c'| for negatives and a conditional
// subtraction per term, as combine_kernel does.
#pragma once

#include "lsr_arith.hpp"
#include "lsr_commit_kernels.hpp"
#include "lsr_commit_rns.hpp"
#include "lsr_commit_tile.hpp"

namespace lsr {

constexpr uint32_t kCombineTerms = 32;        // R: terms between two canonicalisations of the FP64 accumulators (batch.h LSR_COMBINE_TERMS)
constexpr uint32_t kCombineOutputs = 8;       // T: outputs (accumulators per lane) of a workgroup's tile (batch.h LSR_COMBINE_OUTPUTS)
constexpr uint32_t kCombineThreads = 256;     // body words of a tile
static_assert(kCombineTerms * kCombineOutputs == kCombineThreads, "one coefficient per lane and step");
static_assert(1.0 + kCombineTerms * 0.875 <= 32.0, "canonical_f64 takes |v| <= 32 q");

struct CombineJob {
    const uint64_t* rows;        // [(outputs - 1) * term_stride + terms][row_words], device, only read
    const uint64_t* coeffs;      // [outputs][terms] raw 64-bit words, device
    uint64_t* out;               // [outputs][row_words]
    int* status;                 // [outputs]
    uint64_t terms, term_stride, outputs;
    uint64_t row_words;
    uint32_t header_words;       // 5, RNS: 6
    uint32_t body_words;         // (k + 1) n, RNS: twice that
    uint32_t block_words;        // words under the first modulus (== body_words unless RNS)
    uint64_t header[kRnsHeaderWords];   // the header of a row of this context
    uint64_t t;
    uint64_t max_weight;         // the largest sum |c'| the host comparison of lwe_linear_combine accepts
    PlainScale plain;            // t, 1/t for mod_plain
};

// c mod t and the centred form: negative = the residue lies in (t/2, t); magnitude = |c'|
__device__ __forceinline__ double combine_centred(uint64_t word, const CombineJob& job, bool* negative) {
    const double cf = mod_plain(word, job.plain);                  // exact, in [0, t)
    *negative = cf > job.plain.half;                               // half = floor(t/2), as the host's cf > t / 2
    return *negative ? job.plain.t - cf : cf;
}

// u64 flavour: a staged multiplier is |c'| with the sign in the top bit; the residue it acts as under modulus q
constexpr uint64_t kCombineNegative = 1ull << 63;
__device__ __forceinline__ uint64_t combine_residue(uint64_t staged, uint64_t q) {
    const uint64_t mag = staged & ~kCombineNegative;
    return (staged & kCombineNegative) ? q - mag : mag;
}

// grid = outputs.  status[j] = -1 (a term row with a header that is not this context's) / 0 (over the budget) / 1, header of out[j].
__global__ void __launch_bounds__(256) combine_prologue_kernel(CombineJob job) {
    __shared__ unsigned long long weight_sum;
    __shared__ unsigned int any_bad;
    const uint64_t j = blockIdx.x;
    if (threadIdx.x == 0) { weight_sum = 0; any_bad = 0; }
    __syncthreads();
    unsigned long long weight = 0;
    bool bad = false;
    for (uint64_t i = threadIdx.x; i < job.terms; i += 256) {
        const uint64_t* const row = job.rows + (j * job.term_stride + i) * job.row_words;
        for (uint32_t w = 0; w < job.header_words; ++w) bad |= row[w] != job.header[w];
        bool negative;
        weight += (unsigned long long)combine_centred(job.coeffs[j * job.terms + i], job, &negative);     // < t/2 each, terms < 2^32
    }
    // wavefront sums first, one atomic per wavefront
    for (int off = 32; off; off >>= 1) weight += __shfl_xor(weight, off);
    const bool wave_bad = __any(bad);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&weight_sum, weight);
        if (wave_bad) atomicOr(&any_bad, 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) job.status[j] = any_bad ? -1 : (weight_sum <= job.max_weight ? 1 : 0);
    if (threadIdx.x < job.header_words) job.out[j * job.row_words + threadIdx.x] = job.header[threadIdx.x];
}

// grid = (ceil(outputs / kCombineOutputs), ceil(body_words / 256)): neighbouring workgroups share their term words when SHARED;
// launched behind combine_prologue_kernel on the same stream
template <bool F64, bool SHARED>
__global__ void __launch_bounds__(kCombineThreads) combine_body_kernel(CombineJob job, ModParams p0, ModParams p1) {
    constexpr uint32_t R = kCombineTerms, T = kCombineOutputs;
    using elem = typename std::conditional<F64, double, uint64_t>::type;
    __shared__ elem coef[R][T];           // the step's multipliers, term-major: the T values of a term are one 64-byte broadcast read
    const uint32_t x = blockIdx.y * kCombineThreads + threadIdx.x;            // body word of this lane
    const bool live = x < job.body_words;
    const bool second = x >= job.block_words;                                  // RNS: the block under q2
    const ModParams& p = second ? p1 : p0;
    const uint64_t q = p.q;
    const double qd = p.qd, inv_qd = p.inv_qd;
    const uint64_t j0 = (uint64_t)blockIdx.x * T;
    const uint32_t body_bytes = job.body_words * 8u, lane_bytes = x * 8u;     // a dead lane's loads fall outside the resource: dropped, 0
    // staging role of this lane: coefficient (output so, term si) of every step
    const uint32_t so = threadIdx.x / R, si = threadIdx.x % R;
    const uint64_t sj = j0 + so < job.outputs ? j0 + so : job.outputs - 1;
    elem acc[T];
#pragma unroll
    for (uint32_t o = 0; o < T; ++o) acc[o] = 0;
    uint32_t bad = 0;                      // bit o: output o of the tile met a residue >= its modulus
    for (uint64_t base = 0; base < job.terms; base += R) {
        const uint32_t now = (uint32_t)(job.terms - base < R ? job.terms - base : R);
        __syncthreads();                   // the previous step's reads are done
        {
            elem c = 0;
            if (si < now) {
                bool negative;
                const double mag = combine_centred(job.coeffs[sj * job.terms + base + si], job, &negative);
                if constexpr (F64) c = negative ? -mag : mag;
                else c = (uint64_t)mag | (negative ? kCombineNegative : 0);     // the residue q_i - |c'| depends on the reader's modulus
            }
            coef[si][so] = c;
        }
        __syncthreads();
        if constexpr (SHARED) {
#pragma unroll 4
            for (uint32_t i = 0; i < now; ++i) {
                // one resource per term row: its range is the row's body, whatever terms * row_words * 8 comes to
                const rsrc_t r = make_rsrc(job.rows + (base + i) * job.row_words + job.header_words, body_bytes);
                const uint64_t raw = buf_load64(r, lane_bytes, 0);
                if (raw >= q) bad = (1u << T) - 1;
                if constexpr (F64) {
                    const double w = f64_from_u52(raw);
#pragma unroll
                    for (uint32_t o = 0; o < T; ++o) acc[o] += mulmod_f64(w, coef[i][o], qd, inv_qd);
                } else {
#pragma unroll
                    for (uint32_t o = 0; o < T; ++o) {
                        acc[o] += mulmod_barrett128(combine_residue(coef[i][o], q), raw, p);
                        if (acc[o] >= q) acc[o] -= q;
                    }
                }
            }
        } else {
#pragma unroll 2
            for (uint32_t i = 0; i < now; ++i) {
                uint64_t raw[T];
#pragma unroll
                for (uint32_t o = 0; o < T; ++o) {
                    const uint64_t j = j0 + o < job.outputs ? j0 + o : job.outputs - 1;       // a dead output re-reads the last one's rows
                    const rsrc_t r = make_rsrc(job.rows + (j * job.term_stride + base + i) * job.row_words + job.header_words, body_bytes);
                    raw[o] = buf_load64(r, lane_bytes, 0);
                }
#pragma unroll
                for (uint32_t o = 0; o < T; ++o) {
                    if (raw[o] >= q) bad |= 1u << o;
                    if constexpr (F64) {
                        acc[o] += mulmod_f64(f64_from_u52(raw[o]), coef[i][o], qd, inv_qd);
                    } else {
                        acc[o] += mulmod_barrett128(combine_residue(coef[i][o], q), raw[o], p);
                        if (acc[o] >= q) acc[o] -= q;
                    }
                }
            }
        }
        if constexpr (F64) {
#pragma unroll
            for (uint32_t o = 0; o < T; ++o) acc[o] = canonical_f64(acc[o], qd, inv_qd);      // |acc| <= q + 32 * 0.875 q = 29 q
        }
    }
    if (!live) return;
#pragma unroll
    for (uint32_t o = 0; o < T; ++o) {
        const uint64_t j = j0 + o;
        if (j >= job.outputs) break;
        uint64_t word;
        if constexpr (F64) word = u52_from_f64(acc[o]);
        else word = acc[o];
        job.out[j * job.row_words + job.header_words + x] = word;
        if (bad & (1u << o)) atomicMin(&job.status[j], -1);
    }
}

}  // namespace lsr
