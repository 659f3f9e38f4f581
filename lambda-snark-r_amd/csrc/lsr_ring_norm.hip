// Norms and projections of ring vectors (batch.h "norms and projections of ring vectors"): the exact l2 norm squared of
// a vector of ring elements, the Johnson-Lindenstrauss projection p = Pi s whose matrix is expanded from ChaCha20 streams inside the
// kernel that applies it, the rows of Pi as ring elements, and the adjoint Pi^T w of weight vectors (§5k).  Integer code that reads only q and n of the context: one path for every
// flavour, every ring degree and both rings.  No workspace and no part in the context's ring ordering: the device forms enqueue
// kernels in plain stream order and nothing else.
#include <algorithm>

#include "lambda_snark/batch.h"
#include "lsr_ring_call.hpp"
#include "lsr_ring_norm_kernels.hpp"
#include "lsr_runtime.hpp"

namespace lsr {

static_assert(kProjectRows == LSR_RING_PROJECT_ROWS, "batch.h and the kernels agree on the rows of the projection");
static_assert(kProjectRows == kNormThreads, "one lane per row");
static_assert(kProjectSlice % 256 == 0, "a slice is whole stream blocks");
static_assert(kAdjointMaxSets == LSR_RING_PROJECT_ADJOINT_MAX_SETS, "batch.h and the kernels agree on the weight sets of one call");

struct ProjectCall {
    uint64_t len;             // width n
    uint64_t bound;
    uint64_t components;
    uint32_t domain;
    uint64_t index_base;
};

static void l2sq_device(const NttContext& c, const uint64_t* d_x, size_t count, size_t width, uint64_t* d_out, hipStream_t s) {
    const unsigned grid = static_cast<unsigned>(std::min<size_t>(count, 1u << 20));
    hipLaunchKernelGGL(ring_l2sq_kernel, dim3(grid), dim3(kNormThreads), 0, s, d_out, d_x, count, (uint64_t)width << c.logn, c.modulus);
    LSR_HIP(hipGetLastError());
}

// vectors [first, first + count) of a call (vector `first` at d_out, d_status and d_x); d_keys holds the key groups from group_base on
static void project_device(const NttContext& c, int64_t* d_out, int32_t* d_status, const uint64_t* d_x, uint64_t first, uint64_t count,
                           const ProjectCall& call, const uint64_t* d_keys, uint64_t group_base, hipStream_t s) {
    const unsigned sweep = static_cast<unsigned>(std::min<uint64_t>((count * kProjectRows + kNormThreads - 1) / kNormThreads, 256 * 32));
    hipLaunchKernelGGL(ring_project_init_kernel, dim3(sweep), dim3(kNormThreads), 0, s, d_out, d_status, (size_t)count);
    LSR_HIP(hipGetLastError());
    ProjectJob job{};
    job.keys = d_keys;
    job.index_base = call.index_base;
    job.components = call.components;
    job.group_base = group_base;
    job.len = call.len;
    job.q = c.modulus;
    job.bound = call.bound;
    job.slices = static_cast<uint32_t>((call.len + kProjectSlice - 1) / kProjectSlice);      // len <= 2^32: at most 2^21
    job.domain = call.domain;
    // one launch covers at most 2^30 workgroups
    const uint64_t step = std::max<uint64_t>(1, (1ull << 30) / job.slices);
    for (uint64_t j0 = 0; j0 < count; j0 += step) {
        const uint64_t now = std::min(step, count - j0);
        job.out = d_out + j0 * kProjectRows;
        job.status = d_status + j0;
        job.x = d_x + j0 * call.len;
        job.first = first + j0;
        hipLaunchKernelGGL(ring_project_kernel,dim3(static_cast<unsigned>(now * job.slices)), dim3(kNormThreads), 0, s, job);
        LSR_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(ring_project_finish_kernel, dim3(static_cast<unsigned>(std::min<uint64_t>(count, 1u << 20))), dim3(kNormThreads), 0, s, d_out,
                       d_status, (size_t)count);
    LSR_HIP(hipGetLastError());
}

// host buffers through bounded device chunks of whole vectors on the context's work stream; each chunk brings its own key groups
static void host_project(const NttContext& c, int64_t* out, int32_t* status, const uint64_t* x, uint64_t count, const ProjectCall& call,
                         const uint64_t* keys) {
    host_staged(c, count, staging_chunk(count, call.len + kProjectRows),
                {staged_groups(keys, 32, call.components), staged_items(x, nullptr, call.len * 8), staged_items(nullptr, out, kProjectRows * 8),
                 staged_items(nullptr, status, 4)},
                [&](const StagedChunk& k, hipStream_t s) {
                    project_device(c, k.lane<int64_t>(2), k.lane<int32_t>(3), k.lane<const uint64_t>(1), k.first, k.now, call, k.lane<const uint64_t>(0),
                                   k.group_first, s);
                });
}

// rows [rows_first, rows_first + rows) of the matrix of (d_key, index_base) into d_out [rows][len]
static void project_matrix_device(const NttContext& c, uint64_t* d_out, uint64_t rows_first, uint64_t rows, uint64_t len, const uint64_t* d_key,
                                  uint32_t domain, uint64_t index_base, hipStream_t s) {
    ProjectMatrixJob job{};
    job.key = d_key;
    job.len = len;
    job.q = c.modulus;
    job.chunks = static_cast<uint32_t>((len + 65535) >> 16);      // len <= 2^32: at most 2^16, times 256 rows
    job.domain = domain;
    job.out = d_out;
    job.index = index_base + rows_first;
    hipLaunchKernelGGL(ring_project_matrix_kernel, dim3(static_cast<unsigned>(rows * job.chunks)), dim3(kNormThreads), 0, s, job);
    LSR_HIP(hipGetLastError());
}

struct ProjectAdjointCall {
    uint64_t len;             // width n
    uint64_t sets;
    uint64_t components;
    uint32_t conjugate;       // 0 or 1, as the entry point takes it
    uint32_t domain;
    uint64_t index_base;
};

// vectors [first, first + count) of a call (vector `first` at d_out and d_status); d_keys and d_weights hold the groups from
// group_base on.  One kernel, in plain stream order.
static void project_adjoint_device(const NttContext& c, uint64_t* d_out, int32_t* d_status, const uint64_t* d_weights, uint64_t first, uint64_t count,
                                   const ProjectAdjointCall& call, const uint64_t* d_keys, uint64_t group_base, hipStream_t s) {
    ProjectAdjointJob job{};
    job.weights = d_weights;
    job.keys = d_keys;
    job.index_base = call.index_base;
    job.components = call.components;
    job.group_base = group_base;
    job.len = call.len;
    job.n = c.degree;
    job.q = c.modulus;
    job.blocks = static_cast<uint32_t>((call.len + 255) >> 8);      // len <= 2^32: at most 2^24
    job.sets = static_cast<uint32_t>(call.sets);
    job.domain = call.domain;
    job.conjugate = call.conjugate ? (c.cyclic ? 1u : 2u) : 0u;
    const bool wide = c.modulus >> 55 != 0;                          // 256 words below 2^55 sum to less than 2^63
    // one launch covers at most 2^30 workgroups
    const uint64_t step = std::max<uint64_t>(1, (1ull << 30) / job.blocks);
    for (uint64_t j0 = 0; j0 < count; j0 += step) {
        const uint64_t now = std::min(step, count - j0);
        job.out = d_out + j0 * call.sets * call.len;
        job.status = d_status + j0;
        job.first = first + j0;
        const dim3 grid(static_cast<unsigned>(now * job.blocks));
        if (wide) hipLaunchKernelGGL(ring_project_adjoint_kernel<true>, grid, dim3(kNormThreads), 0, s, job);
        else hipLaunchKernelGGL(ring_project_adjoint_kernel<false>, grid, dim3(kNormThreads), 0, s, job);
        LSR_HIP(hipGetLastError());
    }
}

// host buffers through bounded device chunks of whole vectors on the context's work stream; each chunk brings its own key groups and
// weight groups
static void host_project_adjoint(const NttContext& c, uint64_t* out, int32_t* status, const uint64_t* weights, uint64_t count,
                                 const ProjectAdjointCall& call, const uint64_t* keys) {
    const uint64_t per_vector = call.sets * call.len, per_group = call.sets * kProjectRows;
    host_staged(c, count, staging_chunk(count, per_vector),
                {staged_groups(keys, 32, call.components), staged_groups(weights, per_group * 8, call.components),
                 staged_items(nullptr, out, per_vector * 8), staged_items(nullptr, status, 4)},
                [&](const StagedChunk& k, hipStream_t s) {
                    project_adjoint_device(c, k.lane<uint64_t>(2), k.lane<int32_t>(3), k.lane<const uint64_t>(1), k.first, k.now, call,
                                           k.lane<const uint64_t>(0), k.group_first, s);
                });
}

}  // namespace lsr

// ------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------
namespace {

const char* const kOverflow = "the sizes of the buffers overflow size_t";

// step 4 of batch.h's order, without the context: elements = the ring elements of the largest buffer (16 bytes each in the smallest
// ring), projections = vectors with 256 eight-byte outputs each
bool sizes_overflow(size_t a, size_t b, size_t projections) {
    size_t elements = 0, bytes = 0;
    return __builtin_mul_overflow(a, b, &elements) || __builtin_mul_overflow(elements, (size_t)16, &bytes) ||
           __builtin_mul_overflow(projections, (size_t)LSR_RING_PROJECT_ROWS * 8, &bytes);
}

// width n, the length of a vector; throws when it or its `vectors`-fold byte size does not fit
uint64_t vector_length(const NttContext& ctx, size_t vectors, size_t width) {
    size_t len = 0, bytes = 0;
    if (__builtin_mul_overflow(width, (size_t)ctx.degree, &len) || __builtin_mul_overflow(len, (size_t)8, &bytes) || __builtin_mul_overflow(bytes, vectors, &bytes))
        throw std::runtime_error("the sizes of the buffers overflow size_t at this ring degree");
    return len;
}

void require_projectable(uint64_t len) {
    if (len > (1ull << 32))
        throw std::runtime_error("width * n = " + std::to_string(len) + " is above 2^32, the positions one stream's block counter reaches");
}

int l2sq_call(const char* where, const NttContext* ctx, const uint64_t* x, size_t count, size_t width, uint64_t* out, bool device, void* stream) noexcept {
    if (!ctx || !x || !out) return lsr::abi_refuse(where, "NULL context or buffer");
    if (count == 0 || width == 0) return 0;
    if (sizes_overflow(count, width, 0)) return lsr::abi_refuse(where, kOverflow);
    return lsr::abi_guarded(where, [&] {
        const uint64_t len = vector_length(*ctx, count, width);
        lsr::require_apart(out, count * 16, x, count * len * 8, "out overlaps x: the output must not share memory with the operand");
        lsr::require_device();
        if (device) {
            lsr::DeviceGuard guard(ctx->device);
            lsr::l2sq_device(*ctx, x, count, width, out, static_cast<hipStream_t>(stream));
        } else {
            lsr::host_staged(*ctx, out, x, count, 2, len, [&](uint64_t* d_out, const uint64_t* d_in, size_t now, hipStream_t s) {
                lsr::l2sq_device(*ctx, d_in, now, width, d_out, s);
            });
        }
    });
}

int project_call(const char* where, const NttContext* ctx, int64_t* out, int32_t* status, const uint64_t* x, size_t count, size_t width, uint64_t bound,
                 const uint64_t* keys, size_t components, uint32_t domain, uint64_t index_base, bool device, void* stream) noexcept {
    if (!ctx || !out || !status || !x || !keys) return lsr::abi_refuse(where, "NULL context, buffer, keys or status");
    if (components == 0) return lsr::abi_refuse(where, "components must be at least 1");
    if (bound == 0) return lsr::abi_refuse(where, "bound must be at least 1");
    if (count == 0 || width == 0) return 0;
    if (sizes_overflow(count, width, count)) return lsr::abi_refuse(where, kOverflow);
    return lsr::abi_guarded(where, [&] {
        if (bound > ctx->modulus / 2)
            throw std::runtime_error("bound = " + std::to_string(bound) + " is above floor(q / 2) = " + std::to_string(ctx->modulus / 2));
        size_t len = 0;
        if (__builtin_mul_overflow(width, (size_t)ctx->degree, &len)) throw std::runtime_error("width * n overflows size_t");
        require_projectable(len);
        if (bound > (uint64_t)INT64_MAX / len)
            throw std::runtime_error("width * n * bound = " + std::to_string(len) + " * " + std::to_string(bound) + " is above 2^63 - 1: a 64-bit sum would not be exact");
        uint64_t span = 0;
        if (__builtin_mul_overflow((uint64_t)components, (uint64_t)LSR_RING_PROJECT_ROWS, &span) || index_base + span < index_base)
            throw std::runtime_error("index_base + 256 * components overflows 64 bits");
        vector_length(*ctx, count, width);
        const char* const apart = "the outputs must not share memory with the operand";
        lsr::require_apart(out, count * LSR_RING_PROJECT_ROWS * 8, x, count * len * 8, (std::string("out overlaps x: ") + apart).c_str());
        lsr::require_apart(status, count * 4, x, count * len * 8, (std::string("status overlaps x: ") + apart).c_str());
        lsr::require_device();
        // min(components, count): the same streams, and the kernel's 32-bit division applies more often
        const lsr::ProjectCall call{len, bound, std::min<uint64_t>(components, count), domain, index_base};
        if (device) {
            lsr::DeviceGuard guard(ctx->device);
            lsr::project_device(*ctx, out, status, x, 0, count, call, keys, 0, static_cast<hipStream_t>(stream));
        } else {
            lsr::host_project(*ctx, out, status, x, count, call, keys);
        }
    });
}

int project_matrix_call(const char* where, const NttContext* ctx, uint64_t* out, size_t rows_first, size_t rows, size_t width, const uint64_t* key,
                        uint32_t domain, uint64_t index_base, bool device, void* stream) noexcept {
    if (!ctx || !out || !key) return lsr::abi_refuse(where, "NULL context, buffer or key");
    if (rows_first > LSR_RING_PROJECT_ROWS || rows > LSR_RING_PROJECT_ROWS - rows_first)
        return lsr::abi_refuse(where, "rows_first + rows = " + std::to_string(rows_first) + " + " + std::to_string(rows) + " is above " +
                                          std::to_string(LSR_RING_PROJECT_ROWS) + ", the rows of a projection");
    if (rows == 0 || width == 0) return 0;
    if (sizes_overflow(rows, width, 0)) return lsr::abi_refuse(where, kOverflow);
    return lsr::abi_guarded(where, [&] {
        const uint64_t len = vector_length(*ctx, rows, width);
        require_projectable(len);
        if (index_base + LSR_RING_PROJECT_ROWS < index_base) throw std::runtime_error("index_base + 256 overflows 64 bits");
        lsr::require_device();
        if (device) {
            lsr::DeviceGuard guard(ctx->device);
            lsr::project_matrix_device(*ctx, out, rows_first, rows, len, key, domain, index_base, static_cast<hipStream_t>(stream));
        } else {
            // host rows through bounded device chunks; the key goes up once
            lsr::host_staged(*ctx, rows, lsr::staging_chunk(rows, len), {lsr::staged_items(key, nullptr, 0, 32), lsr::staged_items(nullptr, out, len * 8)},
                             [&](const lsr::StagedChunk& k, hipStream_t s) {
                                 lsr::project_matrix_device(*ctx, k.lane<uint64_t>(1), rows_first + k.first, k.now, len, k.lane<const uint64_t>(0), domain, index_base, s);
                             });
        }
    });
}

int project_adjoint_call(const char* where, const NttContext* ctx, uint64_t* out, int32_t* status, const uint64_t* weights, size_t count, size_t sets,
                         size_t width, int conjugate, const uint64_t* keys, size_t components, uint32_t domain, uint64_t index_base, bool device,
                         void* stream) noexcept {
    if (!ctx || !out || !status || !weights || !keys) return lsr::abi_refuse(where, "NULL context, buffer, weights, keys or status");
    if (components == 0) return lsr::abi_refuse(where, "components must be at least 1");
    if (sets == 0 || sets > LSR_RING_PROJECT_ADJOINT_MAX_SETS)
        return lsr::abi_refuse(where, "sets = " + std::to_string(sets) + " is not in 1 .. " + std::to_string(LSR_RING_PROJECT_ADJOINT_MAX_SETS));
    if (conjugate != 0 && conjugate != 1) return lsr::abi_refuse(where, "conjugate = " + std::to_string(conjugate) + " is neither 0 nor 1");
    if (count == 0 || width == 0) return 0;
    size_t outputs = 0;       // count * sets vectors of `width` elements
    if (__builtin_mul_overflow(count, sets, &outputs) || sizes_overflow(outputs, width, 0)) return lsr::abi_refuse(where, kOverflow);
    return lsr::abi_guarded(where, [&] {
        size_t len = 0;
        if (__builtin_mul_overflow(width, (size_t)ctx->degree, &len)) throw std::runtime_error("width * n overflows size_t");
        require_projectable(len);
        uint64_t span = 0;
        if (__builtin_mul_overflow((uint64_t)components, (uint64_t)LSR_RING_PROJECT_ROWS, &span) || index_base + span < index_base)
            throw std::runtime_error("index_base + 256 * components overflows 64 bits");
        vector_length(*ctx, outputs, width);
        const size_t groups = (count - 1) / components + 1;
        size_t weight_bytes = 0;
        if (__builtin_mul_overflow(groups, sets * LSR_RING_PROJECT_ROWS * 8, &weight_bytes))
            throw std::runtime_error("the size of the weights overflows size_t");
        const char* const apart = "the outputs must not share memory with the weights";
        lsr::require_apart(out, outputs * len * 8, weights, weight_bytes, (std::string("out overlaps weights: ") + apart).c_str());
        lsr::require_apart(status, count * 4, weights, weight_bytes, (std::string("status overlaps weights: ") + apart).c_str());
        lsr::require_device();
        // min(components, count): the same streams and groups, and the kernel's 32-bit division applies more often
        const lsr::ProjectAdjointCall call{len, sets, std::min<uint64_t>(components, count), (uint32_t)conjugate, domain, index_base};
        if (device) {
            lsr::DeviceGuard guard(ctx->device);
            lsr::project_adjoint_device(*ctx, out, status, weights, 0, count, call, keys, 0, static_cast<hipStream_t>(stream));
        } else {
            lsr::host_project_adjoint(*ctx, out, status, weights, count, call, keys);
        }
    });
}

}  // namespace

extern "C" {

int lsr_ntt_ring_project_adjoint_batch(const NttContext* ctx, uint64_t* out, int32_t* status, const uint64_t* weights, size_t count, size_t sets,
                                       size_t width, int conjugate, const uint64_t* keys, size_t components, uint32_t domain,
                                       uint64_t index_base) noexcept {
    return project_adjoint_call("lsr_ntt_ring_project_adjoint_batch", ctx, out, status, weights, count, sets, width, conjugate, keys, components, domain,
                                index_base, false, nullptr);
}
int lsr_ntt_ring_project_adjoint_batch_device(const NttContext* ctx, uint64_t* d_out, int32_t* d_status, const uint64_t* d_weights, size_t count,
                                              size_t sets, size_t width, int conjugate, const uint64_t* d_keys, size_t components, uint32_t domain,
                                              uint64_t index_base, void* stream) noexcept {
    return project_adjoint_call("lsr_ntt_ring_project_adjoint_batch_device", ctx, d_out, d_status, d_weights, count, sets, width, conjugate, d_keys,
                                components, domain, index_base, true, stream);
}


int lsr_ntt_ring_l2sq_batch(const NttContext* ctx, const uint64_t* x, size_t count, size_t width, uint64_t* out) noexcept {
    return l2sq_call("lsr_ntt_ring_l2sq_batch", ctx, x, count, width, out, false, nullptr);
}
int lsr_ntt_ring_l2sq_batch_device(const NttContext* ctx, const uint64_t* d_x, size_t count, size_t width, uint64_t* d_out, void* stream) noexcept {
    return l2sq_call("lsr_ntt_ring_l2sq_batch_device", ctx, d_x, count, width, d_out, true, stream);
}

int lsr_ntt_ring_project_batch(const NttContext* ctx, int64_t* out, int32_t* status, const uint64_t* x, size_t count, size_t width, uint64_t bound,
                               const uint64_t* keys, size_t components, uint32_t domain, uint64_t index_base) noexcept {
    return project_call("lsr_ntt_ring_project_batch", ctx, out, status, x, count, width, bound, keys, components, domain, index_base, false, nullptr);
}
int lsr_ntt_ring_project_batch_device(const NttContext* ctx, int64_t* d_out, int32_t* d_status, const uint64_t* d_x, size_t count, size_t width,
                                      uint64_t bound, const uint64_t* d_keys, size_t components, uint32_t domain, uint64_t index_base,
                                      void* stream) noexcept {
    return project_call("lsr_ntt_ring_project_batch_device", ctx, d_out, d_status, d_x, count, width, bound, d_keys, components, domain, index_base, true,
                        stream);
}

int lsr_ntt_ring_project_matrix_batch(const NttContext* ctx, uint64_t* out, size_t rows_first, size_t rows, size_t width, const uint64_t* key,
                                      uint32_t domain, uint64_t index_base) noexcept {
    return project_matrix_call("lsr_ntt_ring_project_matrix_batch", ctx, out, rows_first, rows, width, key, domain, index_base, false, nullptr);
}
int lsr_ntt_ring_project_matrix_batch_device(const NttContext* ctx, uint64_t* d_out, size_t rows_first, size_t rows, size_t width, const uint64_t* d_key,
                                             uint32_t domain, uint64_t index_base, void* stream) noexcept {
    return project_matrix_call("lsr_ntt_ring_project_matrix_batch_device", ctx, d_out, rows_first, rows, width, d_key, domain, index_base, true, stream);
}

}  // extern "C"
