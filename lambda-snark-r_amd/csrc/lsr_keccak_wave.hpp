// Keccak-f[1600] spread over the lanes of a wavefront (device only): ONE 64-bit state word per hardware lane, held as two 32-bit
// registers.  Lane l = 5y + x of a 32-lane half holds A[x][y] for l < 25 (lanes 25..31 idle), so the two halves of a wave64 run two
// sponges side by side and a permutation is 24 x (three dependent cross-lane steps) instead of ~6000 dependent instructions in one
// lane (lsr_keccak.hpp).  Every cross-lane move is a ds_bpermute gather (no LDS memory is touched); per round:
//   theta  C = a ^ g5(a) ^ g10(a) ^ g15(a) ^ g20(a)   4 gathers x 2 registers; g_k reads lane (l + k) mod 25, so every lane ends up
//                                                     with the parity of its own column
//          a ^= C[x-1] ^ rotl1(C[x+1])                2 gathers x 2 registers
//   rho    a right-rotate by a per-lane count: a half swap for counts >= 32 and two v_alignbit_b32
//   pi+chi a = r[s0] ^ (~r[s1] & r[s2])               3 gathers x 2 registers: pi's source-lane table composed with chi's x, x+1, x+2
//   iota   lane 0 xors the round constant (wave-uniform: it sits in scalar registers)
// which is 18 32-bit gathers in three dependent groups (8, 4, 6) and ~25 vector ALU instructions.
//
// The lane table below is the only statement of the layout: the kernel reads it, and tools/experiments/sim_keccak_wave.py parses it
// out of this file, rebuilds it from FIPS 202 and checks a numpy model that gathers with it against hashlib.sha3_256.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "lsr_keccak.hpp"

namespace lsr {

// per lane of a half: up5 up10 up15 up20 | xm1 xp1 | chi0 chi1 chi2 | rotr | padding to 16 bytes (one 128-bit load)
// LSR_KECCAK_WAVE_TABLE_BEGIN
static __device__ const uint8_t kKeccakWaveTable[32][16] = {
    { 5, 10, 15, 20,  4,  1,  0,  6, 12,  0,  0,  0,  0,  0,  0,  0},   // lane 0: A[0][0]
    { 6, 11, 16, 21,  0,  2,  6, 12, 18, 63,  0,  0,  0,  0,  0,  0},   // lane 1: A[1][0]
    { 7, 12, 17, 22,  1,  3, 12, 18, 24,  2,  0,  0,  0,  0,  0,  0},   // lane 2: A[2][0]
    { 8, 13, 18, 23,  2,  4, 18, 24,  0, 36,  0,  0,  0,  0,  0,  0},   // lane 3: A[3][0]
    { 9, 14, 19, 24,  3,  0, 24,  0,  6, 37,  0,  0,  0,  0,  0,  0},   // lane 4: A[4][0]
    {10, 15, 20,  0,  9,  6,  3,  9, 10, 28,  0,  0,  0,  0,  0,  0},   // lane 5: A[0][1]
    {11, 16, 21,  1,  5,  7,  9, 10, 16, 20,  0,  0,  0,  0,  0,  0},   // lane 6: A[1][1]
    {12, 17, 22,  2,  6,  8, 10, 16, 22, 58,  0,  0,  0,  0,  0,  0},   // lane 7: A[2][1]
    {13, 18, 23,  3,  7,  9, 16, 22,  3,  9,  0,  0,  0,  0,  0,  0},   // lane 8: A[3][1]
    {14, 19, 24,  4,  8,  5, 22,  3,  9, 44,  0,  0,  0,  0,  0,  0},   // lane 9: A[4][1]
    {15, 20,  0,  5, 14, 11,  1,  7, 13, 61,  0,  0,  0,  0,  0,  0},   // lane 10: A[0][2]
    {16, 21,  1,  6, 10, 12,  7, 13, 19, 54,  0,  0,  0,  0,  0,  0},   // lane 11: A[1][2]
    {17, 22,  2,  7, 11, 13, 13, 19, 20, 21,  0,  0,  0,  0,  0,  0},   // lane 12: A[2][2]
    {18, 23,  3,  8, 12, 14, 19, 20,  1, 39,  0,  0,  0,  0,  0,  0},   // lane 13: A[3][2]
    {19, 24,  4,  9, 13, 10, 20,  1,  7, 25,  0,  0,  0,  0,  0,  0},   // lane 14: A[4][2]
    {20,  0,  5, 10, 19, 16,  4,  5, 11, 23,  0,  0,  0,  0,  0,  0},   // lane 15: A[0][3]
    {21,  1,  6, 11, 15, 17,  5, 11, 17, 19,  0,  0,  0,  0,  0,  0},   // lane 16: A[1][3]
    {22,  2,  7, 12, 16, 18, 11, 17, 23, 49,  0,  0,  0,  0,  0,  0},   // lane 17: A[2][3]
    {23,  3,  8, 13, 17, 19, 17, 23,  4, 43,  0,  0,  0,  0,  0,  0},   // lane 18: A[3][3]
    {24,  4,  9, 14, 18, 15, 23,  4,  5, 56,  0,  0,  0,  0,  0,  0},   // lane 19: A[4][3]
    { 0,  5, 10, 15, 24, 21,  2,  8, 14, 46,  0,  0,  0,  0,  0,  0},   // lane 20: A[0][4]
    { 1,  6, 11, 16, 20, 22,  8, 14, 15, 62,  0,  0,  0,  0,  0,  0},   // lane 21: A[1][4]
    { 2,  7, 12, 17, 21, 23, 14, 15, 21,  3,  0,  0,  0,  0,  0,  0},   // lane 22: A[2][4]
    { 3,  8, 13, 18, 22, 24, 15, 21,  2,  8,  0,  0,  0,  0,  0,  0},   // lane 23: A[3][4]
    { 4,  9, 14, 19, 23, 20, 21,  2,  8, 50,  0,  0,  0,  0,  0,  0},   // lane 24: A[4][4]
    {25, 25, 25, 25, 25, 25, 25, 25, 25,  0,  0,  0,  0,  0,  0,  0},
    {26, 26, 26, 26, 26, 26, 26, 26, 26,  0,  0,  0,  0,  0,  0,  0},
    {27, 27, 27, 27, 27, 27, 27, 27, 27,  0,  0,  0,  0,  0,  0,  0},
    {28, 28, 28, 28, 28, 28, 28, 28, 28,  0,  0,  0,  0,  0,  0,  0},
    {29, 29, 29, 29, 29, 29, 29, 29, 29,  0,  0,  0,  0,  0,  0,  0},
    {30, 30, 30, 30, 30, 30, 30, 30, 30,  0,  0,  0,  0,  0,  0,  0},
    {31, 31, 31, 31, 31, 31, 31, 31, 31,  0,  0,  0,  0,  0,  0,  0},
};
// LSR_KECCAK_WAVE_TABLE_END

struct KeccakWaveLane {
    int up5, up10, up15, up20, xm1, xp1, chi0, chi1, chi2;   // ds_bpermute byte addresses (4 x source lane of the wavefront)
    uint32_t rotr;                                           // rho as a right-rotate count, 0..63
    uint32_t iota;                                           // all ones on the lane that holds A[0][0]
};

// `lane` is the lane of the wavefront (0..63); sources stay inside the lane's own half
__device__ __forceinline__ KeccakWaveLane keccak_wave_lane(unsigned lane) {
    const uint4 raw = *reinterpret_cast<const uint4*>(kKeccakWaveTable[lane & 31]);
    const int base = (int)(lane & 32);
    auto addr = [&](uint32_t word, int byte) { return (base + (int)((word >> (8 * byte)) & 0xFF)) * 4; };
    KeccakWaveLane t;
    t.up5 = addr(raw.x, 0); t.up10 = addr(raw.x, 1); t.up15 = addr(raw.x, 2); t.up20 = addr(raw.x, 3);
    t.xm1 = addr(raw.y, 0); t.xp1 = addr(raw.y, 1);
    t.chi0 = addr(raw.y, 2); t.chi1 = addr(raw.y, 3); t.chi2 = addr(raw.z, 0);
    t.rotr = (raw.z >> 8) & 0xFF;
    t.iota = (lane & 31) == 0 ? 0xFFFFFFFFu : 0u;
    return t;
}

__device__ __forceinline__ uint32_t keccak_wave_gather(int addr, uint32_t v) { return (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)v); }

// 24 rounds on the word (lo, hi) of this lane; all 64 lanes of the wavefront must be active
__device__ __forceinline__ void keccak_wave_f1600(const KeccakWaveLane& t, uint32_t& lo, uint32_t& hi) {
    const bool swap = t.rotr >= 32;
    const uint32_t rot = t.rotr & 31;
#pragma unroll
    for (int round = 0; round < 24; ++round) {
        const uint64_t rc = keccak_round_constant(round);
        // theta
        const uint32_t c_lo = lo ^ keccak_wave_gather(t.up5, lo) ^ keccak_wave_gather(t.up10, lo) ^ keccak_wave_gather(t.up15, lo) ^ keccak_wave_gather(t.up20, lo);
        const uint32_t c_hi = hi ^ keccak_wave_gather(t.up5, hi) ^ keccak_wave_gather(t.up10, hi) ^ keccak_wave_gather(t.up15, hi) ^ keccak_wave_gather(t.up20, hi);
        const uint32_t m_lo = keccak_wave_gather(t.xm1, c_lo), m_hi = keccak_wave_gather(t.xm1, c_hi);
        const uint32_t p_lo = keccak_wave_gather(t.xp1, c_lo), p_hi = keccak_wave_gather(t.xp1, c_hi);
        lo ^= m_lo ^ __builtin_amdgcn_alignbit(p_lo, p_hi, 31);        // rotl1: {p_lo, p_hi} >> 31
        hi ^= m_hi ^ __builtin_amdgcn_alignbit(p_hi, p_lo, 31);
        // rho: rotate right by rotr = 32 * swap + rot
        const uint32_t s_lo = swap ? hi : lo, s_hi = swap ? lo : hi;
        const uint32_t r_lo = __builtin_amdgcn_alignbit(s_hi, s_lo, rot), r_hi = __builtin_amdgcn_alignbit(s_lo, s_hi, rot);
        // pi and chi
        const uint32_t b0_lo = keccak_wave_gather(t.chi0, r_lo), b1_lo = keccak_wave_gather(t.chi1, r_lo), b2_lo = keccak_wave_gather(t.chi2, r_lo);
        const uint32_t b0_hi = keccak_wave_gather(t.chi0, r_hi), b1_hi = keccak_wave_gather(t.chi1, r_hi), b2_hi = keccak_wave_gather(t.chi2, r_hi);
        // iota
        lo = b0_lo ^ (~b1_lo & b2_lo) ^ ((uint32_t)rc & t.iota);
        hi = b0_hi ^ (~b1_hi & b2_hi) ^ ((uint32_t)(rc >> 32) & t.iota);
    }
}

}  // namespace lsr
