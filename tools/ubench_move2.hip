// Microbenchmark (round 2): pure data movement of the two passes of the n = 2^16 transform, in place, per access variant —
// 8 vs 16 bytes per lane, default vs non-temporal loads / stores — with a little arithmetic so nothing is optimised away.
// Answers VERDICT r1 "What's weak" #4: do b128 accesses or a streaming cache policy move the two-pass floor (1.29 ms)?
//   hipcc --offload-arch=gfx950 -O3 tools/ubench_move2.hip -o tools/bin/ubench_move2
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <algorithm>
#include <vector>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));

template <int W, bool NT> __device__ __forceinline__ void ld(const uint64_t* p, uint64_t (&v)[W]) {
    if constexpr (W == 1) { v[0] = NT ? __builtin_nontemporal_load(p) : *p; }
    else { const u64x2 x = NT ? __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(p)) : *reinterpret_cast<const u64x2*>(p); v[0] = x.x; v[1] = x.y; }
}
template <int W, bool NT> __device__ __forceinline__ void st(uint64_t* p, const uint64_t (&v)[W]) {
    if constexpr (W == 1) { if (NT) __builtin_nontemporal_store(v[0], p); else *p = v[0]; }
    else { u64x2 x; x.x = v[0]; x.y = v[1]; if (NT) __builtin_nontemporal_store(x, reinterpret_cast<u64x2*>(p)); else *reinterpret_cast<u64x2*>(p) = x; }
}

// pass 1: 16 rows 4096 apart (the strided top-bits round); a lane owns W adjacent columns
template <int W, bool NTL, bool NTS>
__global__ void __launch_bounds__(256) pass1(uint64_t* __restrict__ d, size_t total) {
    const size_t g = ((size_t)blockIdx.x * 256 + threadIdx.x) * W;
    if (g >= total / 16) return;
    const size_t idx0 = ((g >> 12) << 16) | (g & 4095);
    uint64_t v[16][W];
#pragma unroll
    for (int k = 0; k < 16; ++k) ld<W, NTL>(d + idx0 + ((size_t)k << 12), v[k]);
#pragma unroll
    for (int k = 0; k < 16; ++k)
#pragma unroll
        for (int w = 0; w < W; ++w) v[k][w] = v[k][w] * 3 + v[(k + 1) & 15][w];
#pragma unroll
    for (int k = 0; k < 16; ++k) st<W, NTS>(d + idx0 + ((size_t)k << 12), v[k]);
}
// pass 2: contiguous 4096-element tiles (256 lanes x 16 residues), a lane owns W adjacent residues per row of 256 W
template <int W, bool NTL, bool NTS>
__global__ void __launch_bounds__(256) pass2(uint64_t* __restrict__ d, size_t total) {
    const size_t base = (size_t)blockIdx.x * 4096 + threadIdx.x * W;
    uint64_t v[16 / W][W];
#pragma unroll
    for (int k = 0; k < 16 / W; ++k) ld<W, NTL>(d + base + (size_t)k * 256 * W, v[k]);
#pragma unroll
    for (int k = 0; k < 16 / W; ++k)
#pragma unroll
        for (int w = 0; w < W; ++w) v[k][w] = v[k][w] * 5 + v[(k + 1) % (16 / W)][w];
#pragma unroll
    for (int k = 0; k < 16 / W; ++k) st<W, NTS>(d + base + (size_t)k * 256 * W, v[k]);
}

// pass 1 of an 8 + 8 split: a 256-lane workgroup owns 16 adjacent columns x 256 rows of a 256 x 256 polynomial (rows 2 KiB
// apart, 128-byte row segments); lane t holds rows (t >> 4) + 16 k of column t & 15
template <bool NTL, bool NTS>
__global__ void __launch_bounds__(256) pass1_cols(uint64_t* __restrict__ d, size_t total) {
    const size_t tile = blockIdx.x;                      // 16 column blocks per polynomial
    const size_t base = ((tile >> 4) << 16) + ((tile & 15) << 4) + (threadIdx.x & 15) + ((size_t)(threadIdx.x >> 4) << 8);
    uint64_t v[16][1];
#pragma unroll
    for (int k = 0; k < 16; ++k) ld<1, NTL>(d + base + ((size_t)k << 12), v[k]);
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k][0] = v[k][0] * 3 + v[(k + 1) & 15][0];
#pragma unroll
    for (int k = 0; k < 16; ++k) st<1, NTS>(d + base + ((size_t)k << 12), v[k]);
}


// round 2, late: wider column tiles for the 8 + 8 split (COLS adjacent columns x 256 rows, COLS*16 lanes: 8*COLS-byte row
// segments instead of 128-byte ones) and deeper strided rounds (2^R rows per lane) for 5 + 11 / 6 + 10 splits
template <int COLS>
__global__ void __launch_bounds__(COLS * 16) pass1_colsw(uint64_t* __restrict__ d, size_t total) {
    constexpr int CB = 256 / COLS;                       // column blocks per polynomial
    const size_t tile = blockIdx.x;
    const uint32_t col = threadIdx.x % COLS, rr = threadIdx.x / COLS;
    const size_t base = ((tile / CB) << 16) + ((tile % CB) * COLS) + col + ((size_t)rr << 8);
    uint64_t v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = d[base + ((size_t)k << 12)];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = v[k] * 3 + v[(k + 1) & 15];
#pragma unroll
    for (int k = 0; k < 16; ++k) d[base + ((size_t)k << 12)] = v[k];
}
template <int R>
__global__ void __launch_bounds__(256) pass1_deep(uint64_t* __restrict__ d, size_t total) {
    constexpr int ROWS = 1 << R, SH = 16 - R;
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= total / ROWS) return;
    const size_t idx0 = ((g >> SH) << 16) | (g & ((1u << SH) - 1));
    uint64_t v[ROWS];
#pragma unroll
    for (int k = 0; k < ROWS; ++k) v[k] = d[idx0 + ((size_t)k << SH)];
#pragma unroll
    for (int k = 0; k < ROWS; ++k) v[k] = v[k] * 3 + v[(k + 1) & (ROWS - 1)];
#pragma unroll
    for (int k = 0; k < ROWS; ++k) d[idx0 + ((size_t)k << SH)] = v[k];
}

// round 18: the intermediate between the two passes stored as 4 + 2 bytes per residue IN PLACE (the fake values keep 48 bits).
// LAYOUT 1, wave cells: the 64 consecutive residues a wavefront touches in one register row own 512 B — bytes [0, 256) the 64 low
//   dwords, [256, 384) the 64 high halfwords, [384, 512) untouched; every access is whole 128-byte lines.  Writers and readers of a cell
//   are one wavefront, so no barrier: in place this is safe because a wavefront's 16 loads have all returned before its first store —
//   every output depends on every input (the sum `s` below keeps that dependence of the real butterflies in the fake arithmetic).
// LAYOUT 2, workgroup cells: the same per 2 KiB row segment of a 256-lane workgroup (1 KiB dwords, 512 B halfwords, 512 B hole); other
//   wavefronts' dwords land on bytes this wavefront reads, so one __syncthreads() separates the loads from the stores.
template <int LAYOUT> __device__ __forceinline__ size_t packed_lo(size_t i) {
    return LAYOUT == 1 ? ((i >> 6) << 9) + ((i & 63) << 2) : ((i >> 8) << 11) + ((i & 255) << 2);
}
template <int LAYOUT> __device__ __forceinline__ size_t packed_hi(size_t i) {
    return LAYOUT == 1 ? ((i >> 6) << 9) + 256 + ((i & 63) << 1) : ((i >> 8) << 11) + 1024 + ((i & 255) << 1);
}
template <int LAYOUT, bool NT> __device__ __forceinline__ uint64_t ld_packed(const uint64_t* d, size_t i) {
    const char* const b = reinterpret_cast<const char*>(d);
    const uint32_t* const pl = reinterpret_cast<const uint32_t*>(b + packed_lo<LAYOUT>(i));
    const int16_t* const ph = reinterpret_cast<const int16_t*>(b + packed_hi<LAYOUT>(i));
    const uint32_t lo = NT ? __builtin_nontemporal_load(pl) : *pl;
    const int16_t hi = NT ? __builtin_nontemporal_load(ph) : *ph;
    return (uint64_t)lo | ((uint64_t)(int64_t)hi << 32);
}
template <int LAYOUT> __device__ __forceinline__ void st_packed(uint64_t* d, size_t i, uint64_t v) {
    char* const b = reinterpret_cast<char*>(d);
    *reinterpret_cast<uint32_t*>(b + packed_lo<LAYOUT>(i)) = (uint32_t)v;
    *reinterpret_cast<uint16_t*>(b + packed_hi<LAYOUT>(i)) = (uint16_t)(v >> 32);
}
// pass 1 (strided rows, plain u64 loads as the library's first pass) writing the packed intermediate over its own operands
template <int LAYOUT>
__global__ void __launch_bounds__(256) pass1_packed(uint64_t* d, size_t total) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= total / 16) return;                         // whole workgroups (total / 16 is a multiple of 256)
    const size_t idx0 = ((g >> 12) << 16) | (g & 4095);
    uint64_t v[16], s = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = d[idx0 + ((size_t)k << 12)];
#pragma unroll
    for (int k = 0; k < 16; ++k) s += v[k];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = v[k] * 3 + s;
    if (LAYOUT == 2) __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) st_packed<LAYOUT>(d, idx0 + ((size_t)k << 12), v[k]);
}
// pass 2 (contiguous tiles) reading the packed intermediate with streaming loads, writing u64 with streaming stores
template <int LAYOUT>
__global__ void __launch_bounds__(256) pass2_packed(uint64_t* d, size_t total) {
    const size_t base = (size_t)blockIdx.x * 4096 + threadIdx.x;
    uint64_t v[16], s = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = ld_packed<LAYOUT, true>(d, base + (size_t)k * 256);
#pragma unroll
    for (int k = 0; k < 16; ++k) s += v[k];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = v[k] * 5 + s;
    if (LAYOUT == 2) __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) __builtin_nontemporal_store(v[k], d + base + (size_t)k * 256);
}

struct Spread { float lo, med, hi; };
template <class F> static Spread timed_spread(F&& launch, hipEvent_t a, hipEvent_t b) {
    std::vector<float> ms;
    for (int rep = 0; rep < 9; ++rep) {
        hipEventRecord(a); launch(); hipEventRecord(b); hipEventSynchronize(b);
        float t; hipEventElapsedTime(&t, a, b); ms.push_back(t);
    }
    std::sort(ms.begin(), ms.end());
    return {ms.front(), ms[ms.size() / 2], ms.back()};
}

template <class F> static float timed(F&& launch, hipEvent_t a, hipEvent_t b) {
    std::vector<float> ms;
    for (int rep = 0; rep < 7; ++rep) {
        hipEventRecord(a); launch(); hipEventRecord(b); hipEventSynchronize(b);
        float t; hipEventElapsedTime(&t, a, b); ms.push_back(t);
    }
    std::sort(ms.begin(), ms.end());
    return ms[ms.size() / 2];
}

int main() {
    const size_t polys = 4096, n = 65536, total = polys * n, chunk_polys = 512, chunk = chunk_polys * n;
    uint64_t* data;
    CK(hipMalloc(&data, total * 8));
    CK(hipMemset(data, 1, total * 8));
    hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
#define RUN1(W, NTL, NTS) timed([&] { for (size_t c = 0; c < polys; c += chunk_polys) hipLaunchKernelGGL((pass1<W, NTL, NTS>), dim3((unsigned)(chunk / 16 / 256 / W)), dim3(256), 0, 0, data + c * n, chunk); }, a, b)
#define RUN2(W, NTL, NTS) timed([&] { for (size_t c = 0; c < polys; c += chunk_polys) hipLaunchKernelGGL((pass2<W, NTL, NTS>), dim3((unsigned)(chunk / 4096)), dim3(256), 0, 0, data + c * n, chunk); }, a, b)
#define RUNB(W1, L1, S1, W2, L2, S2) timed([&] { for (size_t c = 0; c < polys; c += chunk_polys) { \
        hipLaunchKernelGGL((pass1<W1, L1, S1>), dim3((unsigned)(chunk / 16 / 256 / W1)), dim3(256), 0, 0, data + c * n, chunk); \
        hipLaunchKernelGGL((pass2<W2, L2, S2>), dim3((unsigned)(chunk / 4096)), dim3(256), 0, 0, data + c * n, chunk); } }, a, b)
    printf("per 4096 polynomials (2 GiB), in place, 512-polynomial chunks; ms (median of 7)\n");
    printf("pass1 strided  8B  plain          %.3f\n", RUN1(1, false, false));
    printf("pass1 strided 16B  plain          %.3f\n", RUN1(2, false, false));
    printf("pass1 strided  8B  nt-load        %.3f\n", RUN1(1, true, false));
    printf("pass1 strided 16B  nt-load        %.3f\n", RUN1(2, true, false));
    printf("pass1 strided 16B  nt-load+store  %.3f\n", RUN1(2, true, true));
    printf("pass2 tile     8B  plain          %.3f\n", RUN2(1, false, false));
    printf("pass2 tile    16B  plain          %.3f\n", RUN2(2, false, false));
    printf("pass2 tile     8B  nt-store       %.3f\n", RUN2(1, false, true));
    printf("pass2 tile    16B  nt-store       %.3f\n", RUN2(2, false, true));
    printf("pass2 tile    16B  nt-load+store  %.3f\n", RUN2(2, true, true));
    printf("both   8B plain / 8B plain        %.3f   (round-1 floor: 1.29)\n", RUNB(1, false, false, 1, false, false));
    printf("both  16B plain / 16B plain       %.3f\n", RUNB(2, false, false, 2, false, false));
    printf("both  16B nt-load / 16B nt-store  %.3f\n", RUNB(2, true, false, 2, false, true));
    printf("both   8B nt-load / 8B nt-store   %.3f\n", RUNB(1, true, false, 1, false, true));
    printf("both   8B plain / 16B nt-load+store   %.3f\n", RUNB(1, false, false, 2, true, true));
    printf("both   8B plain /  8B nt-load+store   %.3f\n", RUNB(1, false, false, 1, true, true));
    printf("both   8B plain / 16B nt-load          %.3f\n", RUNB(1, false, false, 2, true, false));
    printf("both   8B plain /  8B nt-load          %.3f\n", RUNB(1, false, false, 1, true, false));
    printf("both   8B nt-load / 8B plain           %.3f\n", RUNB(1, true, false, 1, false, false));
    printf("both   8B plain / 8B plain (again)     %.3f\n", RUNB(1, false, false, 1, false, false));
#define RUNC(L1, S1) timed([&] { for (size_t c = 0; c < polys; c += chunk_polys) hipLaunchKernelGGL((pass1_cols<L1, S1>), dim3((unsigned)(chunk / 4096)), dim3(256), 0, 0, data + c * n, chunk); }, a, b)
#define RUNCB(L1, S1, W2, L2, S2) timed([&] { for (size_t c = 0; c < polys; c += chunk_polys) { \
        hipLaunchKernelGGL((pass1_cols<L1, S1>), dim3((unsigned)(chunk / 4096)), dim3(256), 0, 0, data + c * n, chunk); \
        hipLaunchKernelGGL((pass2<W2, L2, S2>), dim3((unsigned)(chunk / 4096)), dim3(256), 0, 0, data + c * n, chunk); } }, a, b)
    printf("pass1 16 cols x 256 rows (8 + 8 split), 8B plain   %.3f\n", RUNC(false, false));
    printf("both  cols-tile plain / 8B nt-load+store            %.3f\n", RUNCB(false, false, 1, true, true));
    printf("both  cols-tile plain / 8B plain                    %.3f\n", RUNCB(false, false, 1, false, false));
    // occupancy sensitivity of the memory-bound passes: dynamic LDS padding limits the resident 256-lane workgroups per CU
    for (unsigned pad : {0u, 36000u, 50000u, 70000u, 100000u}) {
        const float t1 = timed([&] { for (size_t c = 0; c < polys; c += chunk_polys) hipLaunchKernelGGL((pass1<1, false, false>), dim3((unsigned)(chunk / 16 / 256)), dim3(256), pad, 0, data + c * n, chunk); }, a, b);
        const float t2 = timed([&] { for (size_t c = 0; c < polys; c += chunk_polys) hipLaunchKernelGGL((pass1_cols<false, false>), dim3((unsigned)(chunk / 4096)), dim3(256), pad, 0, data + c * n, chunk); }, a, b);
        printf("LDS pad %6u B (<= %u workgroups per CU): strided rows %.3f ms, 16-column tiles %.3f ms\n", pad, pad ? 163840u / pad : 8u, t1, t2);
    }
#define RUNW(COLS) timed([&] { for (size_t c = 0; c < polys; c += chunk_polys) hipLaunchKernelGGL((pass1_colsw<COLS>), dim3((unsigned)(chunk / (COLS * 256))), dim3(COLS * 16), 0, 0, data + c * n, chunk); }, a, b)
#define RUND(R) timed([&] { for (size_t c = 0; c < polys; c += chunk_polys) hipLaunchKernelGGL((pass1_deep<R>), dim3((unsigned)(chunk / (1 << R) / 256)), dim3(256), 0, 0, data + c * n, chunk); }, a, b)
    printf("pass1 16 cols x 256 rows (256 lanes)   %.3f\n", RUNW(16));
    printf("pass1 32 cols x 256 rows (512 lanes)   %.3f\n", RUNW(32));
    printf("pass1 64 cols x 256 rows (1024 lanes)  %.3f\n", RUNW(64));
    printf("pass1 strided 2^4 rows per lane        %.3f\n", RUND(4));
    printf("pass1 strided 2^5 rows per lane        %.3f\n", RUND(5));
    printf("pass1 strided 2^6 rows per lane        %.3f\n", RUND(6));
    // round 18: packed in-place hand-off against the 8-byte one, three interleaved rounds of 9 repeats each (min / median / max)
#define RUNP(LAYOUT) timed_spread([&] { for (size_t c = 0; c < polys; c += chunk_polys) { \
        hipLaunchKernelGGL((pass1_packed<LAYOUT>), dim3((unsigned)(chunk / 16 / 256)), dim3(256), 0, 0, data + c * n, chunk); \
        hipLaunchKernelGGL((pass2_packed<LAYOUT>), dim3((unsigned)(chunk / 4096)), dim3(256), 0, 0, data + c * n, chunk); } }, a, b)
#define RUNB9(W1, L1, S1, W2, L2, S2) timed_spread([&] { for (size_t c = 0; c < polys; c += chunk_polys) { \
        hipLaunchKernelGGL((pass1<W1, L1, S1>), dim3((unsigned)(chunk / 16 / 256 / W1)), dim3(256), 0, 0, data + c * n, chunk); \
        hipLaunchKernelGGL((pass2<W2, L2, S2>), dim3((unsigned)(chunk / 4096)), dim3(256), 0, 0, data + c * n, chunk); } }, a, b)
    for (int round = 0; round < 3; ++round) {
        const Spread u = RUNB9(1, false, false, 1, true, true), w = RUNP(1), g = RUNP(2);
        printf("round %d  both 8B plain / 8B nt-load+store, in place     min %.3f  median %.3f  max %.3f\n", round, u.lo, u.med, u.hi);
        printf("round %d  both 6B wave cells (4 B + 2 B), in place       min %.3f  median %.3f  max %.3f\n", round, w.lo, w.med, w.hi);
        printf("round %d  both 6B workgroup cells (4 B + 2 B), in place  min %.3f  median %.3f  max %.3f\n", round, g.lo, g.med, g.hi);
    }
    CK(hipDeviceSynchronize());
    return 0;
}
