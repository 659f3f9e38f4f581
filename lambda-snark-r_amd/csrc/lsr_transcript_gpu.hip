// A batch of Fiat–Shamir transcripts on the device (rust-api/lambda-snark/src/challenge.rs:102-134), for commitments that are
// already there as rows of one array (lsr_lwe_commit_batch_flat_device).  SHA3-256 is sequential inside a transcript, so there are
// two ways to find parallelism, and a kernel for each:
//   fs_challenge_rows_kernel  ONE LANE per transcript, the 1600-bit state in that lane's registers, no cross-lane traffic.  A launch
//                             takes the time of one transcript (~724 permutations x 13 us at reference size) however few it holds,
//                             and the same time up to 65 536 of them (a wavefront per SIMD): the path for very large batches.
//   fs_challenge_wave_kernel  ONE HALF-WAVEFRONT per transcript, a state word per lane (lsr_keccak_wave.hpp): N transcripts are N/2
//                             wavefronts instead of N/64, and a permutation is 72 short cross-lane steps.  The path for the batch
//                             sizes the provers see; it also chains alpha -> beta (lib.rs:761-768) in one launch.
// lsr_fs_transcript_path() is the rule that picks between them.
#include "lambda_snark/batch.h"
#include "lsr_keccak.hpp"
#include "lsr_keccak_wave.hpp"
#include "lsr_runtime.hpp"

namespace lsr {

// The transcript is tag(20 bytes) || V[0..M) with the virtual word array
//   V = [n_inputs][inputs...][n_words][words...],  M = n_inputs + n_words + 2,
// i.e. its 64-bit units are U[0] = tag[0..8), U[1] = tag[8..16), U[2] = tag[16..20) | lo32(V[0]) << 32 and
// U[t] = hi32(V[t-3]) | lo32(V[t-2]) << 32 for t >= 3; the data ends 4 bytes into unit M + 2.
struct TranscriptView {
    const uint64_t* inputs;
    const uint64_t* words;
    uint64_t n_inputs, n_words;
    __device__ __forceinline__ uint64_t at(uint64_t i) const {
        if (i == 0) return n_inputs;
        if (i <= n_inputs) return inputs[i - 1];
        if (i == n_inputs + 1) return n_words;
        return words[i - n_inputs - 2];
    }
};

__global__ void __launch_bounds__(64) fs_challenge_rows_kernel(const uint64_t* __restrict__ public_inputs, uint64_t n_inputs,
                                                                const uint64_t* __restrict__ words, uint64_t words_per_commitment, uint64_t count,
                                                                uint64_t modulus, uint64_t* __restrict__ alphas, uint64_t* __restrict__ hashes) {
    const uint64_t r = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (r >= count) return;
    const TranscriptView v{public_inputs + r * n_inputs, words + r * words_per_commitment, n_inputs, words_per_commitment};
    const uint64_t M = n_inputs + words_per_commitment + 2;
    const uint64_t tag0 = 0x532D4144424D414CULL, tag1 = 0x462D522D4B52414EULL, tag2 = 0x31762D53ULL;   // "LAMBDA-S" "NARK-R-F" "S-v1"
    uint64_t a[25];
#pragma unroll
    for (int i = 0; i < 25; ++i) a[i] = 0;
    const uint64_t total_bytes = 20 + 8 * M;
    const uint64_t full_blocks = total_bytes / kSha3Rate;
    const uint64_t bulk_from = n_inputs + 2;          // V[i] = words[i - bulk_from] from here on
    uint64_t prev = 0;                                // V[t - 3] of the unit about to be formed
    uint64_t t = 0;
    for (uint64_t blk = 0; blk < full_blocks; ++blk) {
        if (t >= bulk_from + 3) {                     // every unit of this block comes from the commitment words alone
            const uint64_t* w = v.words + (t - 2 - bulk_from);
#pragma unroll
            for (int i = 0; i < 17; ++i) {
                const uint64_t next = w[i];
                a[i] ^= (prev >> 32) | (next << 32);
                prev = next;
            }
            t += 17;
        } else {
#pragma unroll
            for (int i = 0; i < 17; ++i, ++t) {
                uint64_t u;
                if (t == 0) u = tag0;
                else if (t == 1) u = tag1;
                else {
                    const uint64_t next = v.at(t - 2);
                    u = (t == 2 ? tag2 : (prev >> 32)) | (next << 32);
                    prev = next;
                }
                a[i] ^= u;
            }
        }
        keccak_f1600(a);
    }
    // last, padded block: the data ends 4 bytes into one of its units (total = 4 mod 8)
    const uint64_t rem = total_bytes - full_blocks * kSha3Rate;
#pragma unroll
    for (int i = 0; i < 17; ++i, ++t) {
        const uint64_t off = (uint64_t)i * 8;
        uint64_t u = 0;
        if (off + 8 <= rem) {
            if (t == 0) u = tag0;
            else if (t == 1) u = tag1;
            else {
                const uint64_t next = v.at(t - 2);
                u = (t == 2 ? tag2 : (prev >> 32)) | (next << 32);
                prev = next;
            }
        } else if (off < rem) {
            u = (t == 2 ? tag2 : (prev >> 32)) | (0x06ULL << 32);      // 4 data bytes, then the SHA-3 domain byte
        }
        if (i == 16) u ^= 0x8000000000000000ULL;
        a[i] ^= u;
    }
    keccak_f1600(a);
    alphas[r] = a[0] % modulus;                                          // challenge.rs:129-133
    if (hashes) {
#pragma unroll
        for (int i = 0; i < 4; ++i) hashes[r * 4 + i] = a[i];
    }
}

// One half-wavefront per transcript: lane l < 17 of the half absorbs unit U[17 blk + l] of block blk into its state word, the next
// block's loads are issued before the 24 rounds of the current one, and lanes 0..3 end up holding the digest.  In the bulk of a row
// U[t] is the two 32-bit words at 4-byte offset 2 (t - 3 - bulk_from) + 1 of the row: the 17 lanes read 136 contiguous bytes.
// Both transcripts of a wavefront have the same shape (n_inputs, n_words), so every branch on the block number is wave-uniform.
// Chain = true: the same half then hashes V = [1][alpha][n_words][words...] with alpha from its registers and writes beta.
template <bool Chain>
__global__ void __launch_bounds__(64) fs_challenge_wave_kernel(const uint64_t* __restrict__ public_inputs, uint64_t n_inputs,
                                                                const uint64_t* __restrict__ words, uint64_t words_per_commitment, uint64_t count,
                                                                uint64_t modulus, uint64_t* __restrict__ alphas, uint64_t* __restrict__ betas,
                                                                uint64_t* __restrict__ hashes_alpha, uint64_t* __restrict__ hashes_beta) {
    const unsigned lane = threadIdx.x, l = lane & 31;
    uint64_t r = (uint64_t)blockIdx.x * 2 + (lane >> 5);
    const bool live = r < count;                      // the idle half of the last wavefront hashes the last row again and stores nothing
    if (!live) r = count - 1;
    const KeccakWaveLane tab = keccak_wave_lane(lane);
    const uint32_t* in32 = reinterpret_cast<const uint32_t*>(public_inputs + r * n_inputs);
    const uint32_t* w32 = reinterpret_cast<const uint32_t*>(words + r * words_per_commitment);
    uint32_t alpha_lo = 0, alpha_hi = 0;
#pragma unroll 1
    for (int pass = 0; pass < (Chain ? 2 : 1); ++pass) {
        const bool second = Chain && pass == 1;
        const uint64_t n_in = second ? 1 : n_inputs;
        const uint64_t M = n_in + words_per_commitment + 2;
        const uint64_t blocks = (M + 2) / 17 + 1;     // the data ends 4 bytes into unit M + 2, which the last, padded block holds
        const uint64_t bulk_from = n_in + 2;          // V[i] = words[i - bulk_from] from here on
        // 32-bit half `h` of V[i], i < M
        auto v32 = [&](uint64_t i, unsigned h) -> uint32_t {
            if (i == 0) return (uint32_t)(n_in >> (32 * h));
            if (i <= n_in) return second ? (h ? alpha_hi : alpha_lo) : in32[2 * (i - 1) + h];
            if (i == n_in + 1) return (uint32_t)(words_per_commitment >> (32 * h));
            return w32[2 * (i - bulk_from) + h];
        };
        auto load_block = [&](uint64_t blk, uint32_t& u_lo, uint32_t& u_hi) {
            u_lo = u_hi = 0;
            if (l >= 17) return;
            const uint64_t t = 17 * blk + l;
            if (17 * blk >= bulk_from + 3 && blk + 1 < blocks) {        // every unit of this block comes from the commitment words alone
                const uint32_t* p = w32 + 2 * (t - 3 - bulk_from) + 1;
                u_lo = p[0];
                u_hi = p[1];
                return;
            }
            if (t < 2) {
                u_lo = t ? 0x4B52414Eu : 0x424D414Cu;         // "LAMBDA-S" "NARK-R-F" "S-v1" as 32-bit halves
                u_hi = t ? 0x462D522Du : 0x532D4144u;
            } else {
                u_lo = t == 2 ? 0x31762D53u : t <= M + 2 ? v32(t - 3, 1) : 0;
                u_hi = t <= M + 1 ? v32(t - 2, 0) : t == M + 2 ? 0x06u : 0;   // 4 data bytes, then the SHA-3 domain byte
            }
            if (blk + 1 == blocks && l == 16) u_hi ^= 0x80000000u;
        };
        uint32_t lo = 0, hi = 0, n_lo, n_hi;
        load_block(0, n_lo, n_hi);
#pragma unroll 1
        for (uint64_t blk = 0; blk < blocks; ++blk) {
            lo ^= n_lo;
            hi ^= n_hi;
            if (blk + 1 < blocks) load_block(blk + 1, n_lo, n_hi);
            keccak_wave_f1600(tab, lo, hi);
        }
        const uint64_t word = ((uint64_t)hi << 32) | lo;
        const uint64_t challenge = word % modulus;                       // challenge.rs:129-133; meaningful on lane 0 of the half
        uint64_t* out = second ? betas : alphas;
        uint64_t* hashes = second ? hashes_beta : hashes_alpha;
        if (live && l == 0) out[r] = challenge;
        if (live && l < 4 && hashes) hashes[r * 4 + l] = word;
        if (Chain && pass == 0) {
            alpha_lo = keccak_wave_gather((int)(lane & 32) * 4, (uint32_t)challenge);
            alpha_hi = keccak_wave_gather((int)(lane & 32) * 4, (uint32_t)(challenge >> 32));
        }
    }
}

}  // namespace lsr

namespace {

// AUTO's rule, one constant: the smallest measured count at which the lane kernel is the faster one (profiles/r11_transcript_bench.json,
// DESIGN.md §9b).  Below it the wave kernel is LDS-crossbar bound at ~1.6 us per reference-size transcript; from it on the lane
// kernel's flat ~9.4 ms wins.  Single and chained calls cross at the same count, and the count does not move with the row length (both
// kernels' times are proportional to it).
constexpr size_t kFsLaneFromCount = 6144;

int resolve_path(int path, size_t count, size_t words_per_commitment) {
    if (path == LSR_FS_PATH_AUTO) return lsr_fs_transcript_path(count, words_per_commitment);
    return path == LSR_FS_PATH_LANE || path == LSR_FS_PATH_WAVE ? path : -1;
}

void launch_lane(const uint64_t* pub, size_t n_inputs, const uint64_t* words, size_t wpc, size_t count, uint64_t modulus, uint64_t* out, uint8_t* hashes32,
                 hipStream_t s) {
    hipLaunchKernelGGL(lsr::fs_challenge_rows_kernel, dim3(static_cast<unsigned>((count + 63) / 64)), dim3(64), 0, s, pub, (uint64_t)n_inputs, words,
                       (uint64_t)wpc, (uint64_t)count, modulus, out, reinterpret_cast<uint64_t*>(hashes32));
    LSR_HIP(hipGetLastError());
}

template <bool Chain>
void launch_wave(const uint64_t* pub, size_t n_inputs, const uint64_t* words, size_t wpc, size_t count, uint64_t modulus, uint64_t* alphas, uint64_t* betas,
                 uint8_t* hashes_a, uint8_t* hashes_b, hipStream_t s) {
    hipLaunchKernelGGL(lsr::fs_challenge_wave_kernel<Chain>, dim3(static_cast<unsigned>((count + 1) / 2)), dim3(64), 0, s, pub, (uint64_t)n_inputs, words,
                       (uint64_t)wpc, (uint64_t)count, modulus, alphas, betas, reinterpret_cast<uint64_t*>(hashes_a), reinterpret_cast<uint64_t*>(hashes_b));
    LSR_HIP(hipGetLastError());
}

template <class Body>
int guarded(const char* name, Body&& body) noexcept {
    try {
        body();
        return 0;
    } catch (const std::exception& e) {
        lsr::set_last_error(std::string(name) + ": " + e.what());
        return -1;
    } catch (...) {
        return -1;
    }
}

}  // namespace

extern "C" int lsr_fs_transcript_path(size_t count, size_t words_per_commitment) noexcept {
    (void)words_per_commitment;
    return count < kFsLaneFromCount ? LSR_FS_PATH_WAVE : LSR_FS_PATH_LANE;
}

extern "C" int lsr_fs_challenge_batch_device_on(int path, const uint64_t* d_public_inputs, size_t n_inputs, const uint64_t* d_words,
                                                size_t words_per_commitment, size_t count, uint64_t modulus, uint64_t* d_alphas, uint8_t* d_hashes32,
                                                void* stream) noexcept {
    path = resolve_path(path, count, words_per_commitment);
    if (path < 0) {
        lsr::set_last_error("lsr_fs_challenge_batch_device_on: unknown path");
        return -1;
    }
    if ((!d_public_inputs && n_inputs) || !d_words || words_per_commitment == 0 || modulus == 0 || !d_alphas) return -1;
    if (count == 0) return 0;
    return guarded("lsr_fs_challenge_batch_device", [&] {
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (path == LSR_FS_PATH_LANE) launch_lane(d_public_inputs, n_inputs, d_words, words_per_commitment, count, modulus, d_alphas, d_hashes32, s);
        else launch_wave<false>(d_public_inputs, n_inputs, d_words, words_per_commitment, count, modulus, d_alphas, nullptr, d_hashes32, nullptr, s);
    });
}

extern "C" int lsr_fs_challenge_batch_device(const uint64_t* d_public_inputs, size_t n_inputs, const uint64_t* d_words, size_t words_per_commitment,
                                             size_t count, uint64_t modulus, uint64_t* d_alphas, uint8_t* d_hashes32, void* stream) noexcept {
    return lsr_fs_challenge_batch_device_on(LSR_FS_PATH_AUTO, d_public_inputs, n_inputs, d_words, words_per_commitment, count, modulus, d_alphas, d_hashes32,
                                            stream);
}

extern "C" int lsr_fs_challenge_chain_batch_device(int path, const uint64_t* d_public_inputs, size_t n_inputs, const uint64_t* d_words,
                                                   size_t words_per_commitment, size_t count, uint64_t modulus, uint64_t* d_alphas, uint64_t* d_betas,
                                                   uint8_t* d_hashes_alpha32, uint8_t* d_hashes_beta32, void* stream) noexcept {
    path = resolve_path(path, count, words_per_commitment);
    if (path < 0) {
        lsr::set_last_error("lsr_fs_challenge_chain_batch_device: unknown path");
        return -1;
    }
    if ((!d_public_inputs && n_inputs) || !d_words || words_per_commitment == 0 || modulus == 0 || !d_alphas || !d_betas) return -1;
    if (count == 0) return 0;
    return guarded("lsr_fs_challenge_chain_batch_device", [&] {
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (path == LSR_FS_PATH_LANE) {
            launch_lane(d_public_inputs, n_inputs, d_words, words_per_commitment, count, modulus, d_alphas, d_hashes_alpha32, s);
            launch_lane(d_alphas, 1, d_words, words_per_commitment, count, modulus, d_betas, d_hashes_beta32, s);
        } else {
            launch_wave<true>(d_public_inputs, n_inputs, d_words, words_per_commitment, count, modulus, d_alphas, d_betas, d_hashes_alpha32, d_hashes_beta32, s);
        }
    });
}
