// Bit-packed encoding and decoding of short ring elements (batch.h "bit-packed ring elements").  Integer code that reads
// q and n of a context: one path for every flavour, ring and degree.
//   Field of a coefficient x: CENTRED — the low `bits` bits of v = x (x <= (q-1)/2) or x - q; RESIDUE — the low `bits` bits of x; a
//   word >= q contributes its own low bits.  Bit b of field i is stream bit i bits + b, stream bit t is bit t mod 64 of word t / 64.
// Pack, n >= 64: 64 consecutive fields are exactly `bits` words, so the call is count n / 64 independent groups and a tile of
//   kPackThreads P coefficients (P = 2 with 16-byte loads when x is 16-byte aligned, else 1) is 4 P groups = 4 P bits whole output
//   words, wherever the elements begin.  A lane loads its P coefficients coalesced, centres them, tests the two status conditions on
//   that read and builds a unit: its P fields fused when P bits <= 64 (the first fusion step costs nothing), else one unit per field.
//   The units go to LDS (8-byte stores, one pad slot per 16 units: at bits = 1, 2 the readers of consecutive output words are 16 or
//   32 units apart, which unpadded is one bank pair); behind the barrier lane w assembles output word w of the tile from the
//   ceil(64 / unit bits) + 1 units that overlap it and stores it: consecutive lanes, consecutive words.
//   Status: a wavefront's two ballots (a word >= q; a coefficient out of range) decide the elements that lie inside it; an element
//   of several wavefronts goes through four LDS words, and one of several workgroups (n > kPackThreads P) is lowered with atomicMin
//   from 1, which a fill kernel wrote first.
// Pack, n < 64: one lane per element walks its n <= 32 coefficients.  Nothing measures it.
// Unpack, n >= 64: the tile's 4 P bits stream words come in with coalesced 8-byte loads and are staged in LDS (one lane-load per
//   word instead of two to four per lane: fetching each field's words straight from global memory was bound by the address path of
//   the vector memory unit, §5o); a lane owns P coefficients, reads the two staged words that can hold each field (neighbouring
//   lanes read the same or the next word: a broadcast or distinct banks), funnel-shifts without a branch, sign-extends, validates
//   and stores P words coalesced (16 bytes when out is 16-byte aligned).  Statuses as in pack.
// Unpack, n < 64: a lane owns P coefficients and reads the one or two stream words of each field from global memory; the lane that
//   owns an element's last field tests the padding bits.  Nothing measures it.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace lsr {

constexpr int kPackThreads = 256;
constexpr int kPackWaves = kPackThreads / 64;
constexpr int kPackUnits = kPackThreads * 2;                 // the most units of a tile: one per coefficient at P = 2
constexpr int kPackCentred = 0, kPackResidue = 1;            // LSR_RING_PACK_CENTRED, LSR_RING_PACK_RESIDUE

struct PackJob {
    uint64_t* words;          // the packed stream [count][W]
    uint64_t* x;              // the coefficients [count][n]
    int32_t* status;          // [count]
    uint64_t q, half;         // half = (q - 1) / 2
    uint64_t total;           // count n
    uint64_t tile_base;       // this launch covers the tiles from tile_base on
    uint64_t count;
    uint32_t logn;
    uint32_t bits;
    uint32_t wpe;             // W: words per element
};

__device__ __forceinline__ uint32_t pack_unit_slot(uint32_t u) { return u + (u >> 4); }

// the field of word x and what it does to the status
template <int MODE>
__device__ __forceinline__ uint64_t pack_field(uint64_t x, const PackJob& job, uint64_t mask, bool& not_below_q, bool& out_of_range) {
    const bool ge = x >= job.q;
    not_below_q |= ge;
    if constexpr (MODE == kPackCentred) {
        // unsigned compares: q may have 64 bits; v as a two's-complement word
        const uint64_t v = (!ge && x > job.half) ? x - job.q : x;
        const uint64_t bias = 1ull << (job.bits - 1);
        out_of_range |= ((v + bias) >> job.bits) != 0;
        return v & mask;
    } else {
        out_of_range |= (x >> job.bits) != 0;
        return x & mask;
    }
}

// The statuses of the elements a workgroup covers, from every lane's two flags.  lanes_log: log2 of the lanes per element (n / P).
// st: kPackWaves words of LDS.  All lanes of the workgroup call it (it holds a barrier when an element spans wavefronts).
__device__ __forceinline__ void pack_publish_status(const PackJob& job, int32_t* st, bool not_below_q, bool bad, bool live, uint64_t element,
                                                    uint32_t lanes_log) {
    const uint32_t t = threadIdx.x, lane = t & 63u;
    const uint64_t mq = __ballot(not_below_q), mr = __ballot(bad);
    if (lanes_log <= 6) {
        const uint32_t lanes = 1u << lanes_log;
        const uint64_t seg = (lanes == 64 ? ~0ull : ((1ull << lanes) - 1)) << (lane & ~(lanes - 1));
        if ((lane & (lanes - 1)) == 0 && live) job.status[element] = (mq & seg) ? -1 : (mr & seg) ? 0 : 1;
        return;
    }
    if (lane == 0) st[t >> 6] = mq ? -1 : mr ? 0 : 1;
    __syncthreads();
    const uint32_t waves_log = lanes_log - 6;                // wavefronts per element
    if (waves_log <= 2) {                                    // whole elements in this workgroup: lane 64 k owns the one that starts in wavefront k
        const uint32_t waves = 1u << waves_log;
        if (lane == 0 && ((t >> 6) & (waves - 1)) == 0 && live) {
            int32_t s = 1;
            for (uint32_t k = 0; k < waves; ++k) s = min(s, st[(t >> 6) + k]);
            job.status[element] = s;
        }
    } else if (t == 0 && live) {                             // a part of one element: status was filled with 1 before this launch
        const int32_t s = min(min(st[0], st[1]), min(st[2], st[3]));
        if (s < 1) atomicMin(job.status + element, s);
    }
}

__global__ void __launch_bounds__(kPackThreads) ring_pack_fill_status_kernel(int32_t* status, uint64_t count) {
    const uint64_t e = (uint64_t)blockIdx.x * kPackThreads + threadIdx.x;
    if (e < count) status[e] = 1;
}

// n >= 64.  Workgroup = tile of 256 P coefficients = 4 P groups = 4 P bits words of the stream.
template <int P, int MODE>
__global__ void __launch_bounds__(kPackThreads) ring_pack_kernel(PackJob job) {
    __shared__ uint64_t unit[kPackUnits + kPackUnits / 16];
    __shared__ int32_t st[kPackWaves];
    const uint32_t t = threadIdx.x, bits = job.bits;
    const uint64_t tile = job.tile_base + blockIdx.x;
    const uint64_t pos = (tile * kPackThreads + t) * P;      // total is a multiple of 64: a lane's P coefficients are live or not
    const bool live = pos < job.total;
    const uint64_t mask = (1ull << bits) - 1;
    uint64_t x[P] = {};
    if (live) {
        if constexpr (P == 2) {
            const ulonglong2 w = *reinterpret_cast<const ulonglong2*>(job.x + pos);
            x[0] = w.x;
            x[1] = w.y;
        } else {
            x[0] = job.x[pos];
        }
    }
    bool not_below_q = false, bad = false;
    uint64_t f[P];
#pragma unroll
    for (int e = 0; e < P; ++e) f[e] = pack_field<MODE>(x[e], job, mask, not_below_q, bad);
    const bool fused = P == 2 && bits <= 32;
    if (P == 1) unit[pack_unit_slot(t)] = f[0];
    else if (fused) unit[pack_unit_slot(t)] = f[0] | (f[P - 1] << bits);
    else {
        unit[pack_unit_slot(2 * t)] = f[0];
        unit[pack_unit_slot(2 * t + 1)] = f[P - 1];
    }
    pack_publish_status(job, st, not_below_q, bad, live, pos >> job.logn, job.logn - (P == 2 ? 1 : 0));
    __syncthreads();
    // the words of this tile: 4 P bits of them, fewer in the last tile
    const uint64_t tile_first = tile * kPackThreads * P;
    const uint64_t left = job.total - tile_first;
    const uint32_t groups = left < (uint64_t)kPackThreads * P ? (uint32_t)(left >> 6) : kPackWaves * P;
    const uint32_t words = groups * bits, ub = fused ? 2 * bits : bits;
    uint64_t* const out = job.words + (tile_first >> 6) * bits;
    for (uint32_t w = t; w < words; w += kPackThreads) {
        uint32_t u = (64u * w) / ub;
        const uint32_t off = 64u * w - u * ub;
        uint64_t acc = unit[pack_unit_slot(u)] >> off;
        // the tile's stream ends with its last unit: `have` reaches 64 there at the latest
        for (uint32_t have = ub - off; have < 64; have += ub) acc |= unit[pack_unit_slot(++u)] << have;
        out[w] = acc;
    }
}

// n < 64: one lane per element
template <int MODE>
__global__ void __launch_bounds__(kPackThreads) ring_pack_small_kernel(PackJob job) {
    const uint64_t e = job.tile_base + (uint64_t)blockIdx.x * kPackThreads + threadIdx.x;
    if (e >= job.count) return;
    const uint32_t n = 1u << job.logn, bits = job.bits;
    const uint64_t mask = (1ull << bits) - 1;
    const uint64_t* const x = job.x + (e << job.logn);
    uint64_t* out = job.words + e * job.wpe;
    bool not_below_q = false, bad = false;
    uint64_t acc = 0;
    uint32_t have = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t f = pack_field<MODE>(x[i], job, mask, not_below_q, bad);
        acc |= f << have;
        const uint32_t now = have + bits;
        if (now >= 64) {                                     // have >= 1 here: bits < 64
            *out++ = acc;
            acc = now > 64 ? f >> (64 - have) : 0;
            have = now - 64;
        } else {
            have = now;
        }
    }
    if (have) *out = acc;
    job.status[e] = not_below_q ? -1 : bad ? 0 : 1;
}

// the word of field f and whether the field is valid
template <int MODE>
__device__ __forceinline__ uint64_t unpack_word(uint64_t f, const PackJob& job, uint64_t mask, bool& valid) {
    if constexpr (MODE == kPackCentred) {
        if ((f >> (job.bits - 1)) & 1) {
            const uint64_t mag = (~(f | ~mask)) + 1;             // -v, in 1 .. 2^(bits - 1)
            valid = mag <= job.half;
            return job.q - mag;
        }
        valid = f <= job.half;
        return f;
    } else {
        valid = f < job.q;
        return f;
    }
}

// n >= 64.  Workgroup = tile of 256 P coefficients = 4 P bits words of the stream, staged in LDS.
template <int P, int MODE>
__global__ void __launch_bounds__(kPackThreads) ring_unpack_kernel(PackJob job) {
    __shared__ uint64_t staged[kPackWaves * 2 * 63 + 8];         // 4 P bits words and one of zeros behind them
    __shared__ int32_t st[kPackWaves];
    const uint32_t t = threadIdx.x, bits = job.bits;
    const uint64_t tile = job.tile_base + blockIdx.x;
    const uint64_t tile_first = tile * kPackThreads * P, pos = tile_first + (uint64_t)t * P;      // total is a multiple of 64
    const bool live = pos < job.total;
    const uint64_t left = job.total - tile_first;
    const uint32_t groups = left < (uint64_t)kPackThreads * P ? (uint32_t)(left >> 6) : kPackWaves * P;
    const uint32_t words = groups * bits;
    const uint64_t* const in = job.words + (tile_first >> 6) * bits;
    for (uint32_t w = t; w <= words; w += kPackThreads) staged[w] = w < words ? in[w] : 0;
    __syncthreads();
    const uint64_t mask = (1ull << bits) - 1;
    bool bad = false;
    if (live) {
        uint64_t x[P];
#pragma unroll
        for (int e = 0; e < P; ++e) {
            const uint32_t bit = (t * P + e) * bits, w = bit >> 6, off = bit & 63;
            // the high part is shifted by 64 - off in two steps (off = 0: it leaves the word); where the field does not straddle, its bits
            // lie above the mask
            const uint64_t f = ((staged[w] >> off) | ((staged[w + 1] << 1) << (63 - off))) & mask;
            bool valid;
            const uint64_t word = unpack_word<MODE>(f, job, mask, valid);
            bad |= !valid;
            x[e] = valid ? word : 0;
        }
        if constexpr (P == 2) *reinterpret_cast<ulonglong2*>(job.x + pos) = make_ulonglong2(x[0], x[1]);
        else job.x[pos] = x[0];
    }
    pack_publish_status(job, st, false, bad, live, pos >> job.logn, job.logn - (P == 2 ? 1 : 0));
}

// n < 64 (correct at every n).  Workgroup = 256 P coefficients; P = 2 with 16-byte stores when x is 16-byte aligned.
template <int P, int MODE>
__global__ void __launch_bounds__(kPackThreads) ring_unpack_direct_kernel(PackJob job) {
    __shared__ int32_t st[kPackWaves];
    const uint32_t t = threadIdx.x, bits = job.bits, n = 1u << job.logn;
    const uint64_t pos = ((job.tile_base + blockIdx.x) * kPackThreads + t) * P;      // total is even: a lane's P coefficients are live or not
    const bool live = pos < job.total;
    const uint64_t mask = (1ull << bits) - 1;
    const uint64_t element = pos >> job.logn;
    const uint32_t i0 = (uint32_t)(pos & (n - 1));
    bool bad = false;
    uint64_t x[P] = {};
    if (live) {
        const uint64_t* const in = job.words + element * job.wpe;
#pragma unroll
        for (int e = 0; e < P; ++e) {
            const uint64_t bit = (uint64_t)(i0 + e) * bits;  // below 2^22 * 63
            const uint32_t w = (uint32_t)(bit >> 6), off = (uint32_t)(bit & 63);
            uint64_t f = in[w] >> off;
            if (off + bits > 64) f |= in[w + 1] << (64 - off);      // the field straddles: the next word is the element's own
            f &= mask;
            bool valid;
            const uint64_t word = unpack_word<MODE>(f, job, mask, valid);
            bad |= !valid;
            x[e] = valid ? word : 0;
        }
        const uint32_t tail = (uint32_t)(((uint64_t)n * bits) & 63);
        if (tail != 0 && i0 + P == n) bad |= (in[job.wpe - 1] >> tail) != 0;         // the padding bits, n < 64 only
        if constexpr (P == 2) *reinterpret_cast<ulonglong2*>(job.x + pos) = make_ulonglong2(x[0], x[1]);
        else job.x[pos] = x[0];
    }
    pack_publish_status(job, st, false, bad, live, element, job.logn - (P == 2 ? 1 : 0));
}

}  // namespace lsr
