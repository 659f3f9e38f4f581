// Batched ring matrix-vector product y_j = M x_j over Z_q[X]/(X^n + 1) (negacyclic contexts) or Z_q[X]/(X^n - 1) (cyclic contexts)
// with a matrix that stays on the device across calls (LsrRingMatrix, batch.h).
//   n <= 4096: the handle holds M-hat, every entry's forward transform as launch_ntt writes it (computed once, at creation).  ONE
//              launch per call (ntt_tile_ring_matvec, lsr_ring_matvec_kernels.hpp): per tile of the batch axis and block of RB rows,
//              each x_c is transformed once and feeds RB register accumulators; RB inverse transforms at the end.
//   n > 4096:  the handle holds M as given.  Composed route: per chunk of the batch and per row r one ring inner product with M[r]
//              as the shared b (lsr_ntt_ring_dot_batch_device) into a dense chunk of the context's workspace, then a strided copy to
//              y[.][r].  x-hat is recomputed for every row on this route.
#include <algorithm>

#include "lambda_snark/batch.h"
#include "lsr_flavour.hpp"
#include "lsr_ring_call.hpp"
#include "lsr_ring_matrix.hpp"
#include "lsr_ring_matvec_kernels.hpp"
#include "lsr_runtime.hpp"

namespace lsr {

// one tile's x and y ranges are addressed through 32-bit buffer offsets: 4096 cols (rows) words stay below 2^31 bytes
static_assert((uint64_t)LSR_RING_DOT_MAX_TERMS * kTile * 8 <= (1ull << 31), "the x range of one tile must fit a buffer resource");
static_assert((uint64_t)LSR_RING_MATVEC_MAX_ROWS * kTile * 8 < (1ull << 31), "the y range of one tile must fit a buffer resource");
static_assert(LSR_RING_MATVEC_MAX_ROWS <= 65535 && LSR_RING_MATVEC_MAX_MATRIX_BYTES >= (64ull * 256 * 4096 * 8), "grid.y; the 64 x 256 matrix at n = 4096");

static int row_block_of(const NttContext& c) {
    if (c.logn > kTileLog) return 1;   // the composed route goes row by row
    return for_flavour(c, [](auto a) -> int { return MatvecRowBlock<decltype(a)>::value; });
}

template <class A, int LT>
static void matvec_tile(const LsrRingMatrix& m, uint64_t* d_y, const uint64_t* d_x, size_t batch, hipStream_t s) {
    const NttContext& c = *m.ctx;
    constexpr int RB = MatvecRowBlock<A>::value;
    const size_t total = batch << c.logn;
    const dim3 grid(static_cast<unsigned>((total + kTile - 1) / kTile), static_cast<unsigned>((m.rows + RB - 1) / RB));
    hipLaunchKernelGGL((ntt_tile_ring_matvec<A, LT, RB>), grid, dim3(kThreads), 0, s, d_y, d_x, m.data.ptr, total, (uint32_t)m.rows, (uint32_t)m.cols,
                       c.mod, Flavour<A>::fwd(c), Flavour<A>::inv(c), Flavour<A>::consts(c));
}

template <class A>
static void matvec_tile_lt(const LsrRingMatrix& m, uint64_t* d_y, const uint64_t* d_x, size_t batch, hipStream_t s) {
    for_tile_log<1, 12>(m.ctx->logn, [&](auto t) { matvec_tile<A, decltype(t)::value>(m, d_y, d_x, batch, s); });
}

// Polynomials of the composed route's dense chunk: a third of the Infinity Cache budget of a two-pass transform, as each of
// ring_dot's workspace arrays (lsr_ring_dot.hip).  A function of n (and of the process-wide chunk size) only.
static size_t matvec_chunk_polys(const NttContext& c) { return std::max<size_t>(1, (ntt_chunk_bytes() / 3) >> (c.logn + 3)); }

// n > 4096.  Holds ring_matvec_mutex for the whole call: the dense chunk is shared by every matrix of the context.
static void matvec_composed(const LsrRingMatrix& m, uint64_t* d_y, const uint64_t* d_x, size_t batch, hipStream_t s) {
    const NttContext& c = *m.ctx;
    const size_t n = c.degree, chunk = matvec_chunk_polys(c);
    std::lock_guard<std::mutex> lock(c.ring_matvec_mutex);
    uint64_t* const dense = c.ring_matvec_scratch.ptr;
    for (size_t j0 = 0; j0 < batch; j0 += chunk) {
        const size_t now = std::min(chunk, batch - j0);
        for (size_t r = 0; r < m.rows; ++r) {
            // (ordered behind the previous ring call of the context, and so behind this loop's previous copy: same stream)
            if (lsr_ntt_ring_dot_batch_device(&c, dense, d_x + j0 * m.cols * n, m.data.ptr + r * m.cols * n, now, m.cols, 1, s) != 0)
                throw std::runtime_error(std::string("row ") + std::to_string(r) + ": " + last_error_cstr());
            LSR_HIP(hipMemcpy2DAsync(d_y + (j0 * m.rows + r) * n, m.rows * n * 8, dense, n * 8, n * 8, now, hipMemcpyDeviceToDevice, s));
        }
    }
    // The next ring call on the context (which may be a mat-vec on another stream) starts behind the last copy out of `dense`.
    // An empty ring call (wait, then record, under ring_mutex): another thread's ring call may have recorded the event since this
    // call's last inner product released ring_mutex, and the chain of the workspaces' users must stay transitive.
    ring_call(c, c.ring_dot_scratch, 0, false, s, [] {});
}

// One call on the device (caller validated the arguments).
static void matvec_device(const LsrRingMatrix& m, uint64_t* d_y, const uint64_t* d_x, size_t batch, hipStream_t s) {
    const NttContext& c = *m.ctx;
    if (!stream_is_capturing(s)) m.ready.wait(s);
    if (c.logn > kTileLog) {
        matvec_composed(m, d_y, d_x, batch, s);
        return;
    }
    for_flavour(c, [&](auto a) { matvec_tile_lt<decltype(a)>(m, d_y, d_x, batch, s); });
    LSR_HIP(hipGetLastError());
}

// host buffers through bounded device chunks of whole vectors on the context's work stream
static void host_matvec(const LsrRingMatrix& m, uint64_t* y, const uint64_t* x, size_t batch) {
    const size_t n = m.ctx->degree;
    host_staged(*m.ctx, y, x, batch, m.rows * n, m.cols * n,
                [&](uint64_t* d_y, const uint64_t* d_x, size_t now, hipStream_t s) { matvec_device(m, d_y, d_x, now, s); });
}

// device: m is a device pointer, the work is enqueued on `s`; else m is a host pointer and the matrix is complete on return (with
// `fill`: m is not read, the words are written by the kernels fill enqueues)
static LsrRingMatrix* matrix_create(const NttContext& c, const uint64_t* m, size_t rows, size_t cols, bool device, hipStream_t s,
                                    const MatrixFill* fill = nullptr) {
    DeviceGuard guard(c.device);
    const size_t n = c.degree, polys = rows * cols;
    auto mat = std::make_unique<LsrRingMatrix>();
    mat->ctx = &c;
    mat->device = c.device;
    mat->rows = rows;
    mat->cols = cols;
    mat->data.allocate(polys * n);
    if (c.logn > kTileLog) {
        std::lock_guard<std::mutex> lock(c.ring_matvec_mutex);
        if (!c.ring_matvec_scratch.ptr) c.ring_matvec_scratch.allocate(matvec_chunk_polys(c) * n);
    }
    std::unique_lock<std::mutex> staging;
    if (!device) {
        staging = std::unique_lock<std::mutex>(c.staging_mutex);   // serialises use of work_stream(c)
        s = work_stream(c);
        if (fill) (*fill)(mat->data.ptr, s);
        else LSR_HIP(hipMemcpyAsync(mat->data.ptr, m, polys * n * 8, hipMemcpyHostToDevice, s));
        if (c.logn <= kTileLog) launch_ntt(c, mat->data.ptr, polys, false, s);
        LSR_HIP(hipStreamSynchronize(s));
    } else {
        if (c.logn <= kTileLog) launch_ntt(c, mat->data.ptr, polys, false, s, nullptr, nullptr, m);
        else LSR_HIP(hipMemcpyAsync(mat->data.ptr, m, polys * n * 8, hipMemcpyDeviceToDevice, s));
        if (!stream_is_capturing(s)) mat->ready.record(s);
    }
    return mat.release();
}

}  // namespace lsr

// ------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------
// Argument checks of create that need no device and no dereference of ctx, in the documented order: -1 and a message, or 0 to go on.
static int matrix_check(const char* where, const NttContext* ctx, const void* m, size_t rows, size_t cols) {
    if (lsr::refuse_coeff_context(where, ctx)) return -1;
    if (!ctx || !m) return lsr::abi_refuse(where, "NULL context or matrix buffer m");
    if (rows == 0) return lsr::abi_refuse(where, "rows must be at least 1");
    if (cols == 0) return lsr::abi_refuse(where, "cols must be at least 1");
    if (rows > LSR_RING_MATVEC_MAX_ROWS)
        return lsr::abi_refuse(where, "rows = " + std::to_string(rows) + " is above LSR_RING_MATVEC_MAX_ROWS (" + std::to_string(LSR_RING_MATVEC_MAX_ROWS) + ")");
    if (cols > LSR_RING_DOT_MAX_TERMS)
        return lsr::abi_refuse(where, "cols = " + std::to_string(cols) + " is above LSR_RING_DOT_MAX_TERMS (" + std::to_string(LSR_RING_DOT_MAX_TERMS) + ")");
    // (every context has n >= 2: a matrix over the cap at n = 2 is over it on any context)
    if (rows * cols * 2 * 8 > LSR_RING_MATVEC_MAX_MATRIX_BYTES)
        return lsr::abi_refuse(where, "rows * cols = " + std::to_string(rows * cols) + " polynomials are above LSR_RING_MATVEC_MAX_MATRIX_BYTES at any n");
    return 0;
}

static LsrRingMatrix* matrix_create_guarded(const char* where, const NttContext* ctx, const uint64_t* m, size_t rows, size_t cols, bool device,
                                            void* stream, const std::function<void()>* precheck = nullptr,
                                            const lsr::MatrixFill* fill = nullptr) noexcept {
    if (matrix_check(where, ctx, m, rows, cols) != 0) return nullptr;
    LsrRingMatrix* mat = nullptr;
    lsr::abi_guarded(where, [&] {
        lsr::refuse_above_two_pass(*ctx, "ring matrix on a context above n = 131072 is not supported (lsr_cyclic_ntt_context_create_large)");
        if (rows * cols * ctx->degree * 8 > LSR_RING_MATVEC_MAX_MATRIX_BYTES)
            throw std::runtime_error("rows * cols * n * 8 = " + std::to_string(rows * cols * ctx->degree * 8) + " bytes are above LSR_RING_MATVEC_MAX_MATRIX_BYTES (" +
                                     std::to_string(LSR_RING_MATVEC_MAX_MATRIX_BYTES) + ")");
        if (precheck) (*precheck)();
        lsr::require_device();
        mat = lsr::matrix_create(*ctx, m, rows, cols, device, static_cast<hipStream_t>(stream), fill);
    });
    return mat;
}

LsrRingMatrix* lsr::matrix_create_filled(const char* where, const NttContext* ctx, const void* key, size_t rows, size_t cols,
                                         const std::function<void()>& precheck, const MatrixFill& fill) noexcept {
    return matrix_create_guarded(where, ctx, static_cast<const uint64_t*>(key), rows, cols, false, nullptr, &precheck, &fill);
}

// 0: go on; 1: nothing to do; -1: refused
static int matvec_check(const char* where, const LsrRingMatrix* mat, const void* y, const void* x, size_t batch) {
    if (!mat || !y || !x) return lsr::abi_refuse(where, "NULL matrix or buffer");
    return batch == 0 ? 1 : 0;
}

static void matvec_validate(const LsrRingMatrix& mat, const uint64_t* y, const uint64_t* x, size_t batch) {
    const size_t n = mat.ctx->degree;
    lsr::require_apart(y, batch * mat.rows * n * 8, x, batch * mat.cols * n * 8, "y overlaps x: the output must not share memory with the operand");
    lsr::require_device();
}

extern "C" {

LsrRingMatrix* lsr_ntt_ring_matrix_create(const NttContext* ctx, const uint64_t* m, size_t rows, size_t cols) noexcept {
    return matrix_create_guarded("lsr_ntt_ring_matrix_create", ctx, m, rows, cols, false, nullptr);
}

LsrRingMatrix* lsr_ntt_ring_matrix_create_device(const NttContext* ctx, const uint64_t* d_m, size_t rows, size_t cols, void* stream) noexcept {
    return matrix_create_guarded("lsr_ntt_ring_matrix_create_device", ctx, d_m, rows, cols, true, stream);
}

void lsr_ntt_ring_matrix_free(LsrRingMatrix* mat) noexcept {
    if (!mat) return;
    try {
        lsr::DeviceGuard guard(mat->device);
        delete mat;   // (hipFree waits for work still reading the matrix)
    } catch (...) {
        delete mat;
    }
}

size_t lsr_ntt_ring_matrix_rows(const LsrRingMatrix* mat) noexcept { return mat ? mat->rows : 0; }
size_t lsr_ntt_ring_matrix_cols(const LsrRingMatrix* mat) noexcept { return mat ? mat->cols : 0; }
size_t lsr_ntt_ring_matrix_row_block(const LsrRingMatrix* mat) noexcept { return mat ? (size_t)lsr::row_block_of(*mat->ctx) : 0; }

int lsr_ntt_ring_matvec_batch(const LsrRingMatrix* mat, uint64_t* y, const uint64_t* x, size_t batch) noexcept {
    const int rc = matvec_check("lsr_ntt_ring_matvec_batch", mat, y, x, batch);
    if (rc != 0) return rc < 0 ? -1 : 0;
    return lsr::abi_guarded("lsr_ntt_ring_matvec_batch", [&] {
        matvec_validate(*mat, y, x, batch);
        lsr::host_matvec(*mat, y, x, batch);
    });
}

int lsr_ntt_ring_matvec_batch_device(const LsrRingMatrix* mat, uint64_t* d_y, const uint64_t* d_x, size_t batch, void* stream) noexcept {
    const int rc = matvec_check("lsr_ntt_ring_matvec_batch_device", mat, d_y, d_x, batch);
    if (rc != 0) return rc < 0 ? -1 : 0;
    return lsr::abi_guarded("lsr_ntt_ring_matvec_batch_device", [&] {
        matvec_validate(*mat, d_y, d_x, batch);
        lsr::DeviceGuard guard(mat->ctx->device);
        lsr::matvec_device(*mat, d_y, d_x, batch, static_cast<hipStream_t>(stream));
    });
}

}  // extern "C"
