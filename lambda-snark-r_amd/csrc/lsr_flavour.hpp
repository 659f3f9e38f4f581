// Per-flavour views of an NttContext for kernel launches (twiddle tables, round constants), shared by the dispatching translation
// units (lsr_ntt.hip, lsr_ring_mul.hip, lsr_ring_dot.hip, lsr_ring_fold.hip, lsr_ring_matvec.hip, lsr_ring_gadget.hip, lsr_commit.hip).
#pragma once

#include "lsr_ntt_kernels.hpp"
#include "lsr_runtime.hpp"

namespace lsr {

template <class A> struct Flavour;
template <> struct Flavour<ArithF64> {
    static const double* fwd(const NttContext& c) { return c.fwd_f64.ptr; }
    static const double* inv(const NttContext& c) { return c.inv_f64.ptr; }
    static RoundConsts<ArithF64> consts(const NttContext& c) { return {c.n_inv_f64, c.w_last_scaled_f64}; }
};
template <> struct Flavour<ArithU64> {
    static const ShoupOperand* fwd(const NttContext& c) { return c.fwd_u64.ptr; }
    static const ShoupOperand* inv(const NttContext& c) { return c.inv_u64.ptr; }
    static RoundConsts<ArithU64> consts(const NttContext& c) { return {c.n_inv_u64, c.w_last_scaled_u64}; }
};

template <> struct Flavour<ArithGold> {
    static const uint64_t* fwd(const NttContext& c) { return c.fwd_gold.ptr; }
    static const uint64_t* inv(const NttContext& c) { return c.inv_gold.ptr; }
    static RoundConsts<ArithGold> consts(const NttContext& c) { return {c.n_inv_gold, c.w_last_scaled_gold}; }
};

}  // namespace lsr
