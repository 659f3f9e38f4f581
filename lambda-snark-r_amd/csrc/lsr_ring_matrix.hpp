// The resident ring matrix (LsrRingMatrix, batch.h) as the translation units that read it see it: lsr_ring_matvec.hip
// creates it and computes y = M x, lsr_ring_gadget.hip computes y = M G^-1(x) from the same M-hat.
#pragma once

#include <functional>

#include "lsr_ntt_kernels.hpp"
#include "lsr_runtime.hpp"

// The opaque C-ABI handle.  Immutable after creation: calls on one matrix may come from several threads and streams.
struct LsrRingMatrix {
    const NttContext* ctx = nullptr;
    int device = 0;                     // ctx->device, kept here so that freeing the matrix never reads the context
    size_t rows = 0, cols = 0;
    lsr::DeviceBuffer<uint64_t> data;   // [rows][cols][n]: M-hat (n <= 4096) or M (n > 4096)
    lsr::Event ready;                   // recorded by the device form of create: calls on other streams start behind it
};

namespace lsr {

// Rows per workgroup, per flavour, from the compiler's resource report (profiles/r19_ring_matvec_resource_usage.txt).  The rule: the
// largest block that keeps two waves per SIMD at LT = 12 (n = 4096) and has no scratch at any tile size.  Six smaller tile sizes
// (F64 LT 10, Gold LT 8-11, U64 LT 4) then use 3-8 AGPRs beyond 256 VGPRs and run at one wave per SIMD: accepted, not measured.
template <class A> struct MatvecRowBlock;
template <> struct MatvecRowBlock<ArithF64> { static constexpr int value = 4; };
template <> struct MatvecRowBlock<ArithGold> { static constexpr int value = 4; };
template <> struct MatvecRowBlock<ArithU64> { static constexpr int value = 2; };

// lsr_ntt_ring_matrix_create with the matrix words produced on the device (lsr_ring_sample.hip): the same checks in the same order
// with `key` in the place of m, then precheck() (throws to refuse) just before the visible-device check, then fill(d_m, s) enqueues
// the kernels that write M [rows][cols][n] in natural order into the handle's buffer on the context's work stream; at n <= 4096 the
// words are transformed in place behind it.  Complete on return; NULL and lsr_last_error on refusal.
using MatrixFill = std::function<void(uint64_t* d_m, hipStream_t s)>;
LsrRingMatrix* matrix_create_filled(const char* where, const NttContext* ctx, const void* key, size_t rows, size_t cols,
                                    const std::function<void()>& precheck, const MatrixFill& fill) noexcept;

}  // namespace lsr
