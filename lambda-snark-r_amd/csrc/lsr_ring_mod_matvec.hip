// Resident-matrix products under ANY modulus q >= 2 (batch.h "resident matrices under any modulus"): y = M x and
// y = M G^-1(x) in Z_q[X]/(X^n + 1), n <= 4096, on a ring handle (LsrRingMod, lsr_ring_mod.hip).
//   matrix    LsrRingModMatrix keeps, per prime of the handle, the forward transform of the lifted entries: lifted by the streaming
//             kernel into the two buffers, transformed in place on the prime contexts (no scratch at n <= 4096).
//   product   matrix columns are taken in groups that P = p1 p2 can carry — max_terms for a plain x, capacity_bounded(q, n, B/2)
//             for digits — and the outputs in chunks that fit the handle's workspace [2][2^22 words]: whole vectors [vectors][rows][n],
//             or, where one vector's rows n words exceed it, one vector and a range of rows.  Per chunk and group ONE launch of
//             ntt_tile_ring_mod_matvec covers both primes (grid z; one instantiation launches per prime instead, kModMatvecBothPrimes),
//             then one reduce launch into y, accumulating from the second group on.
//   bounded   lsr_ring_mod_matvec_bounded_batch: the plain product with the caller's l-infinity bound on x VERIFIED on
//             the device and a status per vector.  The groups are capacity_bounded(q, n, bound_x) columns; the kernel's checking
//             instantiation holds every word it loads against q and the bound and ORs violations into one flag word per vector of the
//             chunk (the handle's flag words, cleared per chunk: a chunk is at most kRingModMatvecFlagWords vectors); the reduce is
//             ring_mod_gram_reduce_kernel, vector = grid y, which writes zeros over a flagged vector — whatever the earlier groups
//             wrote — and status.  A vector taken in row ranges is checked whole by one storeless pass of ring_mod_gram_lift_kernel
//             before its first reduce, and its tile launches are the unchecked ones; so is a chunk at the sizes where that
//             measured faster or the checking instantiation is a wave short (kModMatvecCheckInTile).
// The bracket of a call, the view of the handle's workspace and the launchers of the check pass and of the gated reduce:
// lsr_ring_mod_call.hpp.  No allocation after create: the device forms capture into a graph from the first call.
#include <algorithm>
#include <memory>

#include "lambda_snark/batch.h"
#include "lsr_flavour.hpp"
#include "lsr_ring_matrix.hpp"
#include "lsr_ring_mod_call.hpp"
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

// Where the bounded product's check runs, decided per instantiation by the compiler's resource report and by measurement
// (profiles/r38_ring_mod_matvec_bounded_resource_usage.txt, profiles/r38_ring_mod_matvec_bounded_bench.json): in the
// tile kernel from n = 512 on, except in the integer flavour at n = 4096, whose checking instantiation is a wave short of its
// unchecked twin.  Elsewhere the chunk's x goes through one storeless check pass and the tile launches are the unchecked ones: at
// n = 64, 128 and 256 the pass measured faster than the check in the tile (n = 256, where the FP64 checking instantiation is a wave
// short as well: 512 us against 589, the plain product 470), at n = 4096 the tile is no slower (2055 against 2074); the sizes between
// follow their neighbours unmeasured.  LSR_MOD_MATVEC_CHECK_IN_TILE = 1 / 0: an experiment build that checks in the tile everywhere /
// nowhere.
#ifndef LSR_MOD_MATVEC_CHECK_IN_TILE
#define LSR_MOD_MATVEC_CHECK_IN_TILE (-1)
#endif
template <class A, int LT>
constexpr bool kModMatvecCheckInTile = LSR_MOD_MATVEC_CHECK_IN_TILE >= 0 ? LSR_MOD_MATVEC_CHECK_IN_TILE != 0
                                                                         : LT >= 9 && !(std::is_same_v<A, ArithU64> && LT == 12);

template <class A>
static bool mod_matvec_checks_in_tile(int logn) {
    bool in_tile = false;
    for_tile_log<1, 12>(logn, [&](auto t) { in_tile = kModMatvecCheckInTile<A, decltype(t)::value>; });
    return in_tile;
}

// CHECK: the launch holds x against q and `bound` and ORs violations into flags[vector of the chunk]
template <class A, bool GADGET, bool CHECK = false>
static void mod_matvec_tile(const LsrRingModMatrix& m, const ModMatvecLaunch& l, const GadgetParams& g, hipStream_t s, uint32_t* flags = nullptr,
                            uint64_t bound = 0) {
    const LsrRingMod& h = *m.h;
    constexpr int RB = MatvecRowBlock<A>::value;
    const size_t n = h.n, total = l.vectors * n, m_row_words = m.cols * n;
    const RingModWorkspace w = ring_mod_workspace(h);
    RingModMatvecPrimes<A> both{};
    for (int i = 0; i < 2; ++i) {
        const NttContext& c = *h.prime[i];
        both.prime[i] = {w.sums[i], m.data[i].ptr + l.row0 * m_row_words, Flavour<A>::fwd(c), Flavour<A>::inv(c), c.mod,
                         Flavour<A>::consts(c), h.lift[i]};
    }
    for_tile_log<1, 12>(h.logn, [&](auto t) {
        constexpr int LT = decltype(t)::value;
        constexpr bool kBoth = kModMatvecBothPrimes<A, LT, GADGET>;
        static_assert(!CHECK || kBoth, "the checking launch takes both primes: the workgroups of prime 0 check");
        if constexpr (CHECK && !kModMatvecCheckInTile<A, LT>) {
            throw std::logic_error("mod_matvec_tile: this size checks in a pass of its own");   // (and its checking instantiation is not built)
        } else {
            const dim3 grid(static_cast<unsigned>((total + kTile - 1) / kTile), static_cast<unsigned>((l.nr + RB - 1) / RB), kBoth ? 2 : 1);
            for (int i = 0; i < (kBoth ? 1 : 2); ++i) {
                if (i) both.prime[0] = both.prime[1];
                hipLaunchKernelGGL((ntt_tile_ring_mod_matvec<A, LT, RB, GADGET, kBoth, CHECK>), grid, dim3(kThreads), 0, s, both, l.x, total,
                                   (uint32_t)l.nr, (uint32_t)l.xcols, (uint32_t)l.col0, (uint32_t)l.ncols, m_row_words, h.q, g, flags, bound);
            }
        }
    });
}

static int mod_row_block(const LsrRingMod& h) { return h.prime[0]->use_f64 ? MatvecRowBlock<ArithF64>::value : MatvecRowBlock<ArithU64>::value; }

// x: [batch][xcols][n]; digits == 0: the plain product (xcols == cols)
template <class A>
static void mod_matvec_enqueue(const LsrRingModMatrix& m, uint64_t* d_y, const uint64_t* d_x, size_t batch, unsigned b, size_t digits, hipStream_t s) {
    const LsrRingMod& h = *m.h;
    const bool gadget = digits != 0;
    const size_t n = h.n, xcols = gadget ? m.cols / digits : m.cols;
    const GadgetParams g = gadget ? gadget_params(h.q, b, digits) : GadgetParams{};
    const size_t capacity = gadget ? ring_mod_capacity_bounded(h.q, h.n, (uint64_t)1 << (b - 1)) : h.max_terms;
    const size_t group_max = std::min(m.cols, capacity);
    const size_t vector_words = m.rows * n;
    const bool whole = vector_words <= kRingModSumWords;
    const size_t chunk = whole ? kRingModSumWords / vector_words : 1, nr_max = whole ? m.rows : kRingModSumWords / n;
    const RingModWorkspace w = ring_mod_workspace(h);
    for (size_t j0 = 0; j0 < batch; j0 += chunk) {
        const size_t now = std::min(chunk, batch - j0);
        for (size_t r0 = 0; r0 < m.rows; r0 += nr_max) {
            const size_t nr = std::min(nr_max, m.rows - r0);
            for (size_t c0 = 0; c0 < m.cols; c0 += group_max) {
                const ModMatvecLaunch l{d_x + j0 * xcols * n, now, r0, nr, c0, std::min(group_max, m.cols - c0), xcols};
                for_bool(gadget, [&](auto ga) { mod_matvec_tile<A, decltype(ga)::value>(m, l, g, s); });
                LSR_HIP(hipGetLastError());
                // (the chunk's words are contiguous in y: whole vectors, or rows r0 .. r0 + nr of one)
                launch_reduce(h, d_y + (j0 * m.rows + r0) * n, w.sums[0], w.sums[1], now * nr * n, c0 > 0, s);
            }
        }
    }
}

// The vectors of one chunk of a bounded product: one flag word each
constexpr size_t kRingModMatvecFlagWords = 2 * kRingModFoldFlagWords;
static_assert(kRingModMatvecFlagWords <= 65535, "the vectors of a chunk are one grid axis of the reduce");

// The bounded plain product: x [batch][cols][n] held against q and bound_x (0: none), status [batch].  mod_matvec_enqueue's loops with
// the groups of the verified bound, the chunk capped by the flag words and the gated reduce.
template <class A>
static void mod_matvec_bounded_enqueue(const LsrRingModMatrix& m, uint64_t* d_y, int32_t* d_status, const uint64_t* d_x, size_t batch, uint64_t bound_x,
                                       hipStream_t s) {
    const LsrRingMod& h = *m.h;
    const size_t n = h.n;
    const uint64_t bound = bound_x ? bound_x : h.q >> 1;
    const size_t group_max = std::min(m.cols, ring_mod_capacity_bounded(h.q, h.n, bound));    // the capacity is >= max_terms >= 1
    const size_t vector_words = m.rows * n;
    const bool whole = vector_words <= kRingModSumWords;
    const size_t chunk = whole ? std::min(kRingModSumWords / vector_words, kRingModMatvecFlagWords) : 1, nr_max = whole ? m.rows : kRingModSumWords / n;
    const RingModWorkspace w = ring_mod_workspace(h);
    // a vector in row ranges (now == 1) needs its flags before its first reduce: the check pass, whatever the instantiation
    const bool in_tile = whole && mod_matvec_checks_in_tile<A>(h.logn);
    for (size_t j0 = 0; j0 < batch; j0 += chunk) {
        const size_t now = std::min(chunk, batch - j0);
        const uint64_t* const xj = d_x + j0 * m.cols * n;
        zero_words_async(reinterpret_cast<uint64_t*>(w.flags), (now + 1) / 2, s);
        if (!in_tile) ring_mod_check_pass(h, xj, w.flags, m.cols * n, now, m.cols * n, bound, s);
        for (size_t r0 = 0; r0 < m.rows; r0 += nr_max) {
            const size_t nr = std::min(nr_max, m.rows - r0);
            for (size_t c0 = 0; c0 < m.cols; c0 += group_max) {
                const ModMatvecLaunch l{xj, now, r0, nr, c0, std::min(group_max, m.cols - c0), m.cols};
                for_bool(in_tile, [&](auto check) { mod_matvec_tile<A, false, decltype(check)::value>(m, l, GadgetParams{}, s, w.flags, bound); });
                LSR_HIP(hipGetLastError());
                // [now][nr n] of y: one chunk of whole vectors, or one row range of one vector
                ring_mod_gated_reduce(h, d_y + (j0 * m.rows + r0) * n, d_status + j0, w.sums[0], w.sums[1], w.flags, nr * n, now, c0 > 0, s);
            }
        }
    }
}

// One call on the device (caller validated the arguments) in the handle's bracket (ring_mod_call), behind the matrix's ready event.
// d_status: the bounded product (b and digits 0), else the plain or the gadget product.
static void mod_matvec_device(const LsrRingModMatrix& m, uint64_t* d_y, const uint64_t* d_x, size_t batch, unsigned b, size_t digits, hipStream_t s,
                              int32_t* d_status = nullptr, uint64_t bound_x = 0) {
    ring_mod_call(*m.h, s, false, [&] {
        if (!stream_is_capturing(s)) m.ready.wait(s);
        for_ring_mod_flavour(*m.h, [&](auto a) {
            if (d_status) mod_matvec_bounded_enqueue<decltype(a)>(m, d_y, d_status, d_x, batch, bound_x, s);
            else mod_matvec_enqueue<decltype(a)>(m, d_y, d_x, batch, b, digits, s);
        });
    });
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

// batch.h's refusals of the bounded product in its order
int matvec_bounded_call(const char* where, const LsrRingModMatrix* mat, uint64_t* y, int32_t* status, const uint64_t* x, size_t batch, uint64_t bound_x,
                        bool device, void* stream) noexcept {
    if (!mat || !y || !status || !x) return lsr::abi_refuse(where, "NULL matrix, buffer or status");
    const uint64_t half = mat->q >> 1;
    if (bound_x > half)
        return lsr::abi_refuse(where, "bound_x = " + std::to_string(bound_x) + " is above floor(q / 2) = " + std::to_string(half) + " (0 states none)");
    if (batch == 0) return 0;
    return lsr::abi_guarded(where, [&] {
        const size_t n = mat->n, x_bytes = batch * mat->cols * n * 8, y_bytes = batch * mat->rows * n * 8, status_bytes = batch * sizeof(int32_t);
        lsr::require_apart(y, y_bytes, x, x_bytes, "y overlaps x: the output must not share memory with the operand");
        lsr::require_apart(status, status_bytes, x, x_bytes, "status overlaps x: the output must not share memory with the operand");
        lsr::require_apart(status, status_bytes, y, y_bytes, "status overlaps y: the two outputs must not share memory");
        lsr::require_device();
        if (device) {
            lsr::DeviceGuard guard(mat->device);
            lsr::mod_matvec_device(*mat, y, x, batch, 0, 0, static_cast<hipStream_t>(stream), status, bound_x);
            return;
        }
        const size_t x_words = mat->cols * n, y_words = mat->rows * n;
        lsr::host_staged(*mat->h->prime[0], batch, lsr::staging_chunk(batch, x_words + y_words + 1),
                         {lsr::staged_items(x, nullptr, x_words * 8), lsr::staged_items(nullptr, y, y_words * 8),
                          lsr::staged_items(nullptr, status, sizeof(int32_t))},
                         [&](const lsr::StagedChunk& k, hipStream_t s) {
                             lsr::mod_matvec_device(*mat, k.lane<uint64_t>(1), k.lane<const uint64_t>(0), k.now, 0, 0, s, k.lane<int32_t>(2), bound_x);
                         });
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
int lsr_ring_mod_matvec_bounded_batch(const LsrRingModMatrix* mat, uint64_t* y, int32_t* status, const uint64_t* x, size_t batch,
                                      uint64_t bound_x) noexcept {
    return matvec_bounded_call("lsr_ring_mod_matvec_bounded_batch", mat, y, status, x, batch, bound_x, false, nullptr);
}
int lsr_ring_mod_matvec_bounded_batch_device(const LsrRingModMatrix* mat, uint64_t* d_y, int32_t* d_status, const uint64_t* d_x, size_t batch,
                                             uint64_t bound_x, void* stream) noexcept {
    return matvec_bounded_call("lsr_ring_mod_matvec_bounded_batch_device", mat, d_y, d_status, d_x, batch, bound_x, true, stream);
}

}  // extern "C"
