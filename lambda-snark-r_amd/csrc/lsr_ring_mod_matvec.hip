// Resident-matrix products under ANY modulus q >= 2 (batch.h "resident matrices under any modulus"): y = M x and
// y = M G^-1(x) in Z_q[X]/(X^n + 1), n <= 4096, on a ring handle (LsrRingMod, lsr_ring_mod.hip).
//   matrix    LsrRingModMatrix keeps, per prime of the handle, the forward transform of the lifted entries: lifted by the streaming
//             kernel into the two buffers, transformed in place on the prime contexts (no scratch at n <= 4096).
//   product   matrix columns are taken in groups that P = p1 p2 can carry — max_terms for a plain x, capacity_bounded(q, n, B/2)
//             for digits — and the outputs in chunks that fit the handle's workspace [2][2^22 words]: whole vectors [vectors][rows][n],
//             or, where one vector's rows n words exceed it, one vector and a range of rows.  Per chunk and group ONE launch of
//             ntt_tile_ring_mod_matvec covers both primes (grid z; one instantiation launches per prime instead, kModMatvecBothPrimes),
//             then one reduce launch into y, accumulating from the second group on.
// No allocation after create: the device forms capture into a graph from the first call.
#include <algorithm>
#include <memory>

#include "lambda_snark/batch.h"
#include "lsr_flavour.hpp"
#include "lsr_ring_call.hpp"
#include "lsr_ring_matrix.hpp"
#include "lsr_ring_mod.hpp"
#include "lsr_ring_mod_matvec_kernels.hpp"
#include "lsr_runtime.hpp"

// The opaque C-ABI handle.  Immutable after creation: calls on one matrix may come from several threads and streams.
struct LsrRingModMatrix {
    // q, rows, cols and n stay the first fields: the accessors and the refusals that precede device work read nothing else
    uint64_t q = 0;
    size_t rows = 0, cols = 0;
    uint32_t n = 0;
    int device = 0;
    const LsrRingMod* h = nullptr;
    lsr::DeviceBuffer<uint64_t> data[2];   // per prime [rows][cols][n]: M-hat of the lifted entries
    lsr::Event ready;                      // recorded by the device form of create: calls on other streams start behind it
};

namespace lsr {

static_assert((uint64_t)LSR_RING_DOT_MAX_TERMS * kTile * 8 <= (1ull << 31), "the x range of one tile must fit a buffer resource");
static_assert((uint64_t)LSR_RING_MATVEC_MAX_ROWS * kTile * 8 < (1ull << 31), "the y range of one tile must fit a buffer resource");
static_assert(kRingModSumWords >= kTile, "a chunk holds at least one row of one vector");

// one chunk and one group: both primes
struct ModMatvecLaunch {
    const uint64_t* x;       // the chunk's first vector
    size_t vectors;
    size_t row0, nr;         // the chunk's rows
    size_t col0, ncols;      // the group's matrix columns
    size_t xcols;
};

// Both primes in one launch (grid z = 2), or one launch per prime with the prime's arguments at a fixed place: decided per
// instantiation by the compiler's resource report (profiles/r33_ring_mod_matvec_resource_usage.txt).  The indexed
// arguments cost a wave in one instantiation only: the integer flavour's gadget kernel at LT = 11 (one AGPR past 256 VGPRs).
template <class A, int LT, bool GADGET>
constexpr bool kModMatvecBothPrimes = !(std::is_same_v<A, ArithU64> && GADGET && LT == 11);

template <class A, bool GADGET>
static void mod_matvec_tile(const LsrRingModMatrix& m, const ModMatvecLaunch& l, const GadgetParams& g, hipStream_t s) {
    const LsrRingMod& h = *m.h;
    constexpr int RB = MatvecRowBlock<A>::value;
    const size_t n = h.n, total = l.vectors * n, m_row_words = m.cols * n;
    RingModMatvecPrimes<A> both{};
    for (int i = 0; i < 2; ++i) {
        const NttContext& c = *h.prime[i];
        both.prime[i] = {h.ws.ptr + i * kRingModSumWords, m.data[i].ptr + l.row0 * m_row_words, Flavour<A>::fwd(c), Flavour<A>::inv(c), c.mod,
                         Flavour<A>::consts(c), h.lift[i]};
    }
    for_tile_log<1, 12>(h.logn, [&](auto t) {
        constexpr int LT = decltype(t)::value;
        constexpr bool kBoth = kModMatvecBothPrimes<A, LT, GADGET>;
        const dim3 grid(static_cast<unsigned>((total + kTile - 1) / kTile), static_cast<unsigned>((l.nr + RB - 1) / RB), kBoth ? 2 : 1);
        for (int i = 0; i < (kBoth ? 1 : 2); ++i) {
            if (i) both.prime[0] = both.prime[1];
            hipLaunchKernelGGL((ntt_tile_ring_mod_matvec<A, LT, RB, GADGET, kBoth>), grid, dim3(kThreads), 0, s, both, l.x, total, (uint32_t)l.nr,
                               (uint32_t)l.xcols, (uint32_t)l.col0, (uint32_t)l.ncols, m_row_words, h.q, g);
        }
    });
}

// the flavour of the prime contexts: FP64 unless the process forces the integer kernels, the same for both (one process-wide switch)
static bool primes_use_f64(const LsrRingMod& h) {
    if (h.prime[0]->use_f64 != h.prime[1]->use_f64) throw std::runtime_error("the two prime contexts run different kernel flavours");
    return h.prime[0]->use_f64;
}

static int mod_row_block(const LsrRingMod& h) { return h.prime[0]->use_f64 ? MatvecRowBlock<ArithF64>::value : MatvecRowBlock<ArithU64>::value; }

// x: [batch][xcols][n]; digits == 0: the plain product (xcols == cols)
static void mod_matvec_enqueue(const LsrRingModMatrix& m, uint64_t* d_y, const uint64_t* d_x, size_t batch, unsigned b, size_t digits, hipStream_t s) {
    const LsrRingMod& h = *m.h;
    const bool gadget = digits != 0, f64 = primes_use_f64(h);
    const size_t n = h.n, xcols = gadget ? m.cols / digits : m.cols;
    const GadgetParams g = gadget ? gadget_params(h.q, b, digits) : GadgetParams{};
    const size_t capacity = gadget ? ring_mod_capacity_bounded(h.q, h.n, (uint64_t)1 << (b - 1)) : h.max_terms;
    const size_t group_max = std::min(m.cols, capacity);
    const size_t vector_words = m.rows * n;
    const bool whole = vector_words <= kRingModSumWords;
    const size_t chunk = whole ? kRingModSumWords / vector_words : 1, nr_max = whole ? m.rows : kRingModSumWords / n;
    const uint64_t *sum0 = h.ws.ptr, *sum1 = h.ws.ptr + kRingModSumWords;
    for (size_t j0 = 0; j0 < batch; j0 += chunk) {
        const size_t now = std::min(chunk, batch - j0);
        for (size_t r0 = 0; r0 < m.rows; r0 += nr_max) {
            const size_t nr = std::min(nr_max, m.rows - r0);
            for (size_t c0 = 0; c0 < m.cols; c0 += group_max) {
                const ModMatvecLaunch l{d_x + j0 * xcols * n, now, r0, nr, c0, std::min(group_max, m.cols - c0), xcols};
                for_bool(gadget, [&](auto ga) {
                    if (f64) mod_matvec_tile<ArithF64, decltype(ga)::value>(m, l, g, s);
                    else mod_matvec_tile<ArithU64, decltype(ga)::value>(m, l, g, s);
                });
                LSR_HIP(hipGetLastError());
                // (the chunk's words are contiguous in y: whole vectors, or rows r0 .. r0 + nr of one)
                launch_reduce(h, d_y + (j0 * m.rows + r0) * n, sum0, sum1, now * nr * n, c0 > 0, s);
            }
        }
    }
}

// One call on the device (caller validated the arguments): ring_mod_dot_device's brackets on the handle's mutex and event.
static void mod_matvec_device(const LsrRingModMatrix& m, uint64_t* d_y, const uint64_t* d_x, size_t batch, unsigned b, size_t digits, hipStream_t s) {
    const LsrRingMod& h = *m.h;
    std::lock_guard<std::mutex> lock(h.mutex);
    const bool capturing = stream_is_capturing(s);
    if (!capturing) {
        m.ready.wait(s);
        h.event.wait(s);
    }
    mod_matvec_enqueue(m, d_y, d_x, batch, b, digits, s);
    if (!capturing) h.event.record(s);
}

enum class MatrixSource { kHost, kDevice, kSeeded };
struct SeededMatrix {
    const uint64_t* key;
    uint32_t domain;
    uint64_t index_base;
};

// kHost: m is a host pointer, the matrix is complete on return; kDevice: m is a device pointer, the work is enqueued on `s`;
// kSeeded: m is not read, the words are sampled on the device, complete on return
static LsrRingModMatrix* mod_matrix_create(const LsrRingMod& h, const uint64_t* m, size_t rows, size_t cols, MatrixSource source, hipStream_t s,
                                           const SeededMatrix* seeded) {
    DeviceGuard guard(h.device);
    const size_t n = h.n, polys = rows * cols, words = polys * n;
    auto mat = std::make_unique<LsrRingModMatrix>();
    mat->q = h.q;
    mat->rows = rows;
    mat->cols = cols;
    mat->n = h.n;
    mat->device = h.device;
    mat->h = &h;
    for (int i = 0; i < 2; ++i) mat->data[i].allocate(words);
    uint64_t* const d0 = mat->data[0].ptr;
    uint64_t* const d1 = mat->data[1].ptr;
    if (source == MatrixSource::kDevice) {
        launch_lift(h, 0, d0, m, words, s);
        launch_lift(h, 1, d1, m, words, s);
        for (int i = 0; i < 2; ++i) launch_ntt(*h.prime[i], mat->data[i].ptr, polys, false, s);
        if (!stream_is_capturing(s)) mat->ready.record(s);
        return mat.release();
    }
    const NttContext& c = *h.prime[0];
    DeviceBuffer<uint64_t> d_key;
    std::lock_guard<std::mutex> staging(c.staging_mutex);   // serialises use of work_stream(c)
    s = work_stream(c);
    if (source == MatrixSource::kSeeded) {
        d_key.allocate(4);
        LSR_HIP(hipMemcpyAsync(d_key.ptr, seeded->key, 32, hipMemcpyHostToDevice, s));
        sample_uniform_device(h.q, h.logn, d0, polys, d_key.ptr, seeded->domain, seeded->index_base, s);
    } else {
        LSR_HIP(hipMemcpyAsync(d0, m, words * 8, hipMemcpyHostToDevice, s));
    }
    // the words mod q sit in the first prime's buffer: out of place into the second, then in place in the first
    launch_lift(h, 1, d1, d0, words, s);
    launch_lift(h, 0, d0, d0, words, s);
    for (int i = 0; i < 2; ++i) launch_ntt(*h.prime[i], mat->data[i].ptr, polys, false, s);
    LSR_HIP(hipStreamSynchronize(s));
    return mat.release();
}

}  // namespace lsr

// ------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------
namespace {

// batch.h's refusals of create in its order; steps 1-6 read nothing of the handle, 7 and 8 its n
LsrRingModMatrix* create_call(const char* where, const LsrRingMod* h, const uint64_t* m, size_t rows, size_t cols, lsr::MatrixSource source, void* stream,
                              const lsr::SeededMatrix* seeded) noexcept {
    auto refuse = [&](const std::string& why) -> LsrRingModMatrix* { return lsr::abi_refuse(where, why), nullptr; };
    if (!h || !(seeded ? static_cast<const void*>(seeded->key) : static_cast<const void*>(m)))
        return refuse(seeded ? "NULL handle or key" : "NULL handle or matrix buffer m");
    if (rows == 0) return refuse("rows must be at least 1");
    if (cols == 0) return refuse("cols must be at least 1");
    if (rows > LSR_RING_MATVEC_MAX_ROWS)
        return refuse("rows = " + std::to_string(rows) + " is above LSR_RING_MATVEC_MAX_ROWS (" + std::to_string(LSR_RING_MATVEC_MAX_ROWS) + ")");
    if (cols > LSR_RING_DOT_MAX_TERMS)
        return refuse("cols = " + std::to_string(cols) + " is above LSR_RING_DOT_MAX_TERMS (" + std::to_string(LSR_RING_DOT_MAX_TERMS) + ")");
    // (every handle has n >= 2: a matrix over the cap at n = 2 is over it on any handle)
    if (rows * cols * 2 * 8 > LSR_RING_MATVEC_MAX_MATRIX_BYTES)
        return refuse("rows * cols = " + std::to_string(rows * cols) + " polynomials are above LSR_RING_MATVEC_MAX_MATRIX_BYTES at any n");
    LsrRingModMatrix* mat = nullptr;
    lsr::abi_guarded(where, [&] {
        const size_t n = h->n;
        if (n > lsr::kTile)
            throw std::runtime_error("n = " + std::to_string(n) + " is above 4096, where the product has no fused form: lsr_ring_mod_lift_batch_device M for "
                                     "each prime, lsr_ntt_ring_matrix_create_device on lsr_ring_mod_prime_context(h, 0) and (h, 1), lift x for each "
                                     "prime, run lsr_ntt_ring_matvec_batch_device on the two matrices and pass the two results to "
                                     "lsr_ring_mod_reduce_batch_device, with the columns in groups of at most lsr_ring_mod_max_terms(h) reduced with accumulate");
        if (rows * cols * n * 8 > LSR_RING_MATVEC_MAX_MATRIX_BYTES)
            throw std::runtime_error("rows * cols * n * 8 = " + std::to_string(rows * cols * n * 8) + " bytes per prime are above LSR_RING_MATVEC_MAX_MATRIX_BYTES (" +
                                     std::to_string(LSR_RING_MATVEC_MAX_MATRIX_BYTES) + ")");
        if (seeded && seeded->index_base + rows * cols < seeded->index_base) throw std::runtime_error("index_base + rows * cols overflows 64 bits");
        lsr::require_device();
        mat = lsr::mod_matrix_create(*h, m, rows, cols, source, static_cast<hipStream_t>(stream), seeded);
    });
    return mat;
}

// batch.h's refusals of the products in its order; digits == 0 with gadget == false: the plain product
int matvec_call(const char* where, const LsrRingModMatrix* mat, uint64_t* y, const uint64_t* x, size_t batch, bool gadget, unsigned b, size_t digits,
                bool device, void* stream) noexcept {
    if (!mat || !y || !x) return lsr::abi_refuse(where, "NULL matrix or buffer");
    if (gadget) {
        if (b < 2 || b > 32) return lsr::abi_refuse(where, "base_log2 = " + std::to_string(b) + " is outside [2, 32]");
        if (digits == 0) return lsr::abi_refuse(where, "digits must be at least 1");
        if (digits > 64 / b)
            return lsr::abi_refuse(where, "base_log2 * digits is above 64 (base_log2 = " + std::to_string(b) + ", digits = " + std::to_string(digits) + ")");
        if (!lsr::gadget_admissible(mat->q, b, digits)) {
            const uint64_t need = lsr_ring_gadget_min_digits(mat->q, b);
            return lsr::abi_refuse(where, "(base_log2 = " + std::to_string(b) + ", digits = " + std::to_string(digits) + ") is not admissible for q = " +
                                              std::to_string(mat->q) +
                                              (need ? ": the digits do not cover the centred residues; lsr_ring_gadget_min_digits gives " + std::to_string(need)
                                                    : ": no digit count is admissible at this base (lsr_ring_gadget_min_digits gives 0)"));
        }
        if (mat->cols % digits != 0)
            return lsr::abi_refuse(where, "cols = " + std::to_string(mat->cols) + " of the matrix is not a multiple of digits = " + std::to_string(digits));
    }
    if (batch == 0) return 0;
    return lsr::abi_guarded(where, [&] {
        const size_t n = mat->n, xcols = gadget ? mat->cols / digits : mat->cols;
        lsr::require_apart(y, batch * mat->rows * n * 8, x, batch * xcols * n * 8, "y overlaps x: the output must not share memory with the operand");
        lsr::require_device();
        const size_t d = gadget ? digits : 0;
        if (device) {
            lsr::DeviceGuard guard(mat->device);
            lsr::mod_matvec_device(*mat, y, x, batch, b, d, static_cast<hipStream_t>(stream));
        } else {
            lsr::host_staged(*mat->h->prime[0], y, x, batch, mat->rows * n, xcols * n, [&](uint64_t* d_y, const uint64_t* d_x, size_t now, hipStream_t s) {
                lsr::mod_matvec_device(*mat, d_y, d_x, now, b, d, s);
            });
        }
    });
}

}  // namespace

extern "C" {

LsrRingModMatrix* lsr_ring_mod_matrix_create(const LsrRingMod* h, const uint64_t* m, size_t rows, size_t cols) noexcept {
    return create_call("lsr_ring_mod_matrix_create", h, m, rows, cols, lsr::MatrixSource::kHost, nullptr, nullptr);
}

LsrRingModMatrix* lsr_ring_mod_matrix_create_device(const LsrRingMod* h, const uint64_t* d_m, size_t rows, size_t cols, void* stream) noexcept {
    return create_call("lsr_ring_mod_matrix_create_device", h, d_m, rows, cols, lsr::MatrixSource::kDevice, stream, nullptr);
}

LsrRingModMatrix* lsr_ring_mod_matrix_create_seeded(const LsrRingMod* h, const uint64_t key[4], uint32_t domain, uint64_t index_base, size_t rows,
                                                    size_t cols) noexcept {
    const lsr::SeededMatrix seeded{key, domain, index_base};
    return create_call("lsr_ring_mod_matrix_create_seeded", h, nullptr, rows, cols, lsr::MatrixSource::kSeeded, nullptr, &seeded);
}

void lsr_ring_mod_matrix_free(LsrRingModMatrix* mat) noexcept {
    if (!mat) return;
    try {
        lsr::DeviceGuard guard(mat->device);
        mat->ready.sync();
        mat->h->event.sync();        // a product still in flight reads the matrix
        delete mat;
    } catch (...) {
        delete mat;
    }
}

size_t lsr_ring_mod_matrix_rows(const LsrRingModMatrix* mat) noexcept { return mat ? mat->rows : 0; }
size_t lsr_ring_mod_matrix_cols(const LsrRingModMatrix* mat) noexcept { return mat ? mat->cols : 0; }
size_t lsr_ring_mod_matrix_row_block(const LsrRingModMatrix* mat) noexcept { return mat && mat->h ? (size_t)lsr::mod_row_block(*mat->h) : 0; }

int lsr_ring_mod_matvec_batch(const LsrRingModMatrix* mat, uint64_t* y, const uint64_t* x, size_t batch) noexcept {
    return matvec_call("lsr_ring_mod_matvec_batch", mat, y, x, batch, false, 0, 0, false, nullptr);
}
int lsr_ring_mod_matvec_batch_device(const LsrRingModMatrix* mat, uint64_t* d_y, const uint64_t* d_x, size_t batch, void* stream) noexcept {
    return matvec_call("lsr_ring_mod_matvec_batch_device", mat, d_y, d_x, batch, false, 0, 0, true, stream);
}
int lsr_ring_mod_matvec_gadget_batch(const LsrRingModMatrix* mat, uint64_t* y, const uint64_t* x, size_t batch, unsigned base_log2, size_t digits) noexcept {
    return matvec_call("lsr_ring_mod_matvec_gadget_batch", mat, y, x, batch, true, base_log2, digits, false, nullptr);
}
int lsr_ring_mod_matvec_gadget_batch_device(const LsrRingModMatrix* mat, uint64_t* d_y, const uint64_t* d_x, size_t batch, unsigned base_log2, size_t digits,
                                            void* stream) noexcept {
    return matvec_call("lsr_ring_mod_matvec_gadget_batch_device", mat, d_y, d_x, batch, true, base_log2, digits, true, stream);
}

}  // extern "C"
