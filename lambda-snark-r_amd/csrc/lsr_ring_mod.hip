// Ring products in Z_q[X]/(X^n + 1) for ANY modulus q >= 2, prime or not (batch.h "ring products under any modulus"):
// a handle owns two negacyclic contexts of the 44-bit NTT primes p1, p2 of the RNS commitments (rns_moduli_for) and computes the
// exact INTEGER negacyclic product of centred operands from its residues mod P = p1 p2, then reduces that integer mod q.
//   lift / reduce   the two streaming kernels (lsr_ring_mod_kernels.hpp), public at every n the handle admits: with the prime
//                   contexts they put every bilinear call of the toolkit under q by composition.
//   mul / dot       n <= 4096, fused: per chunk of outputs and group of terms ONE ntt_tile_ring_dot_lift launch per prime (the operands
//                   are centred and re-based as the tile kernel reads them, lsr_ring_galois_kernels.hpp) into the handle's workspace
//                   [2][chunk][n], then one reduce launch into c.  A shared b is lifted into the workspace and transformed once per
//                   prime and group (launch_ntt; at n <= 4096 a transform needs none of the prime context's scratch).  Groups hold at
//                   most max_terms terms — what P can carry — and every group after the first is reduced with `accumulate`.
//   dot_galois      c_j = sum_i sigma_g(a_{j,i}) b_{j,i}: dot with ntt_tile_ring_dot_lift_galois in place of the tile
//                   kernel, which fetches the words of a through the permutation before it lifts them; same groups, same workspace.
//   coeff context   an NttContext of (q, n) without twiddle tables, owned by the handle (create_coeff_context, lsr_ntt.hip): the
//                   coefficient-wise calls of the toolkit run on it under q, every call that transforms refuses it (§5t).
// The workspace is sized by n alone and allocated with the handle, so the device forms capture into a graph from the first call.
// Its layout (ring_mod_workspace) and the bracket of a call (ring_mod_call): lsr_ring_mod_call.hpp.
#include <algorithm>
#include <cstring>

#include "lambda_snark/batch.h"
#include "lsr_flavour.hpp"
#include "lsr_ring_mod_call.hpp"
#include "lsr_ring_workspace.hpp"
#include "lsr_runtime.hpp"

namespace lsr {

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static unsigned stream_grid(size_t count, bool vec) {
    const size_t items = vec ? (count + 1) / 2 : count;
    return static_cast<unsigned>(std::max<size_t>(1, std::min<size_t>((items + kRingModThreads - 1) / kRingModThreads, 8192)));
}

void launch_lift(const LsrRingMod& h, int i, uint64_t* d_out, const uint64_t* d_x, size_t count, hipStream_t s) {
    const bool vec = aligned16(d_out) && aligned16(d_x);
    for_bool(vec, [&](auto v) {
        hipLaunchKernelGGL(ring_mod_lift_kernel<decltype(v)::value>, dim3(stream_grid(count, vec)), dim3(kRingModThreads), 0, s, d_out, d_x, count, h.lift[i]);
    });
    LSR_HIP(hipGetLastError());
}

void launch_reduce(const LsrRingMod& h, uint64_t* d_out, const uint64_t* d_r0, const uint64_t* d_r1, size_t count, bool accumulate, hipStream_t s) {
    const bool vec = aligned16(d_out) && aligned16(d_r0) && aligned16(d_r1);
    for_bool(vec, [&](auto v) {
        for_bool(accumulate, [&](auto acc) {
            hipLaunchKernelGGL((ring_mod_reduce_kernel<decltype(v)::value, decltype(acc)::value>), dim3(stream_grid(count, vec)), dim3(kRingModThreads), 0, s,
                               d_out, d_r0, d_r1, count, h.rc, h.prime[1]->mod, h.pq);
        });
    });
    LSR_HIP(hipGetLastError());
}

struct DotLiftOperands {
    uint64_t* c;
    const uint64_t *a, *b;
    size_t total;        // words of c
    uint32_t nterms;
    size_t a_os, b_os;   // words between consecutive outputs' term-i polynomials
};

// one prime's launch: the flavour of that prime's context (FP64 unless the process forces the integer kernels).  g: the words of a
// go through sigma_g (the twisted inner product), NULL for the plain one
template <bool BHAT>
static void dot_lift_tile(const NttContext& c, const LiftSource& lift, const GaloisParams* g, const DotLiftOperands& o, hipStream_t s) {
    const unsigned grid = static_cast<unsigned>((o.total + kTile - 1) / kTile);
    auto launch = [&](auto a) {
        using A = decltype(a);
        for_tile_log<1, 12>(c.logn, [&](auto t) {
            constexpr int LT = decltype(t)::value;
            if (g)
                hipLaunchKernelGGL((ntt_tile_ring_dot_lift_galois<A, LT, BHAT>), dim3(grid), dim3(kThreads), 0, s, o.c, o.a, o.b, o.total, o.nterms, o.a_os, o.b_os,
                                   kRingDotFirst | kRingDotLast, *g, lift, c.mod, Flavour<A>::fwd(c), Flavour<A>::inv(c), Flavour<A>::consts(c));
            else
                hipLaunchKernelGGL((ntt_tile_ring_dot_lift<A, LT, BHAT>), dim3(grid), dim3(kThreads), 0, s, o.c, o.a, o.b, o.total, o.nterms, o.a_os, o.b_os,
                                   kRingDotFirst | kRingDotLast, lift, c.mod, Flavour<A>::fwd(c), Flavour<A>::inv(c), Flavour<A>::consts(c));
        });
    };
    if (c.use_f64) launch(ArithF64{});
    else launch(ArithU64{});
}

// n <= 4096.  a: [batch][terms][n] with `terms` the stride of an output's terms; accumulate: c already holds partial sums mod q.
// g (or NULL): sigma_g on the words of a.  It permutes and negates the centred coefficients, so a group carries what it carries without.
static void ring_mod_dot_enqueue(const LsrRingMod& h, uint64_t* d_c, const uint64_t* d_a, const uint64_t* d_b, size_t batch, size_t terms, bool shared_b,
                                 bool accumulate, const GaloisParams* g, hipStream_t s) {
    const size_t n = h.n;
    const RingModWorkspace w = ring_mod_workspace(h);
    const size_t group_max = std::min({terms, h.max_terms, shared_b ? h.bhat_rows : terms});
    for (size_t i0 = 0; i0 < terms; i0 += group_max) {
        const size_t group = std::min(group_max, terms - i0);
        if (shared_b) {
            for (int i = 0; i < 2; ++i) {
                launch_lift(h, i, w.bhat[i], d_b + i0 * n, group * n, s);
                launch_ntt(*h.prime[i], w.bhat[i], group, false, s);
            }
        }
        for (size_t j0 = 0; j0 < batch; j0 += h.chunk) {
            const size_t now = std::min(h.chunk, batch - j0), off = (j0 * terms + i0) * n;
            for (int i = 0; i < 2; ++i) {
                if (shared_b) dot_lift_tile<true>(*h.prime[i], h.lift[i], g, {w.sums[i], d_a + off, w.bhat[i], now * n, (uint32_t)group, terms * n, 0}, s);
                else dot_lift_tile<false>(*h.prime[i], h.lift[i], g, {w.sums[i], d_a + off, d_b + off, now * n, (uint32_t)group, terms * n, terms * n}, s);
            }
            launch_reduce(h, d_c + j0 * n, w.sums[0], w.sums[1], now * n, accumulate || i0 > 0, s);
        }
    }
}

// One call on the device (caller validated the arguments) in the handle's bracket (ring_mod_call).  g: 0 for the plain product, else
// the odd Galois element below 2 n applied to a
static void ring_mod_dot_device(const LsrRingMod& h, uint64_t* d_c, const uint64_t* d_a, const uint64_t* d_b, size_t batch, size_t terms, size_t b_rows,
                                bool accumulate, uint64_t g, hipStream_t s) {
    // g^-1 mod 2 n by Newton's iteration, which doubles the correct low bits (g is its own inverse mod 8), as lsr_ring_galois.hip
    uint32_t inv = (uint32_t)g;
    for (int i = 0; i < 4; ++i) inv *= 2u - (uint32_t)g * inv;
    const GaloisParams gp{inv & (2u * h.n - 1u), 2u * h.n - 1u};
    ring_mod_call(h, s, false, [&] { ring_mod_dot_enqueue(h, d_c, d_a, d_b, batch, terms, b_rows == 1 && batch > 1, accumulate, g ? &gp : nullptr, s); });
}

static size_t mul_or_max(size_t x, size_t y) {
    size_t r = 0;
    return __builtin_mul_overflow(x, y, &r) ? SIZE_MAX : r;
}

}  // namespace lsr

// ------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------
namespace {

// mul is dot with terms == 1, except that c may be a or b itself.  g: 0 for mul and dot, else the Galois element of dot_galois (1 is
// the plain product through the same kernel).  Refusals in batch.h's order.
int ring_mod_dot_call(const char* where, const LsrRingMod* h, uint64_t* c, const uint64_t* a, const uint64_t* b, size_t batch, size_t terms, size_t b_rows,
                      bool is_mul, bool device, void* stream, bool galois = false, uint64_t g = 0) noexcept {
    if (!h || !c || !a || !b) return lsr::abi_refuse(where, "NULL handle or buffer");
    if (b_rows != 1 && b_rows != batch)
        return lsr::abi_refuse(where, "b_rows must be 1 or batch (" + std::to_string(batch) + "), got " + std::to_string(b_rows));
    if (terms == 0) return lsr::abi_refuse(where, "terms must be at least 1");
    if (galois && (g & 1) == 0) return lsr::abi_refuse(where, "g = " + std::to_string(g) + " is even: a Galois element is odd");
    if (batch == 0) return 0;
    return lsr::abi_guarded(where, [&] {
        const size_t n = h->n, poly_bytes = n * 8;
        if (galois && g >= 2 * (uint64_t)n) throw std::runtime_error("g = " + std::to_string(g) + " is not below 2 n = " + std::to_string(2 * (uint64_t)n));
        if (galois && h->logn > lsr::kTileLog)
            throw std::runtime_error("n = " + std::to_string(n) + " is above 4096, where the twisted inner product has no fused form: "
                                     "lsr_ring_mod_lift_batch_device both operands for each prime, run lsr_ntt_ring_dot_galois_batch_device on "
                                     "lsr_ring_mod_prime_context(h, 0) and (h, 1), and pass the two results to lsr_ring_mod_reduce_batch_device");
        if (h->logn > lsr::kTileLog)
            throw std::runtime_error("n = " + std::to_string(n) + " is above 4096, where the product has no fused form: lsr_ring_mod_lift_batch_device "
                                     "both operands for each prime, run lsr_ntt_ring_" + (is_mul ? "mul" : "dot") + "_batch_device on "
                                     "lsr_ring_mod_prime_context(h, 0) and (h, 1), and pass the two results to lsr_ring_mod_reduce_batch_device");
        if (terms > LSR_RING_DOT_MAX_TERMS)
            throw std::runtime_error("terms = " + std::to_string(terms) + " is above LSR_RING_DOT_MAX_TERMS (" + std::to_string(LSR_RING_DOT_MAX_TERMS) + ")");
        const size_t a_polys = lsr::mul_or_max(batch, terms), b_polys = lsr::mul_or_max(b_rows, terms);
        if (a_polys == SIZE_MAX || lsr::mul_or_max(a_polys, poly_bytes) == SIZE_MAX) throw std::runtime_error("the sizes of the buffers overflow size_t");
        if (!(is_mul && c == a)) lsr::require_apart(c, batch * poly_bytes, a, a_polys * poly_bytes, "c overlaps a: the output must not share memory with an operand");
        if (!(is_mul && c == b && b_rows == batch))
            lsr::require_apart(c, batch * poly_bytes, b, b_polys * poly_bytes, "c overlaps b: the output must not share memory with an operand");
        lsr::require_device();
        if (device) {
            lsr::DeviceGuard guard(h->device);
            lsr::ring_mod_dot_device(*h, c, a, b, batch, terms, b_rows, false, g, static_cast<hipStream_t>(stream));
        } else {
            lsr::host_staged_dot(*h->prime[0], c, a, b, batch, terms, b_rows,
                                 [&](uint64_t* d_c, const uint64_t* d_a, const uint64_t* d_b, size_t now, size_t group, size_t rows, hipStream_t s, bool first,
                                     bool) { lsr::ring_mod_dot_device(*h, d_c, d_a, d_b, now, group, rows, !first, g, s); });
        }
    });
}

// the checks the two streaming calls share after their NULL checks: 1 for the empty call, -1 refused, 0 to go on
int stream_check(const char* where, size_t count) {
    if (count == 0) return 1;
    if (lsr::mul_or_max(count, 8) == SIZE_MAX) return lsr::abi_refuse(where, "the sizes of the buffers overflow size_t");
    return 0;
}
void require_same_or_apart(const void* out, const void* in, size_t bytes, const char* message) {
    if (out != in) lsr::require_apart(out, bytes, in, bytes, message);
}
void require_words(std::initializer_list<const void*> buffers) {
    for (const void* p : buffers)
        if (reinterpret_cast<uintptr_t>(p) & 7u) throw std::runtime_error("a buffer is not 8-byte aligned");
}

}  // namespace

extern "C" {

int lsr_ring_mod_primes(uint32_t n, uint64_t primes[2]) noexcept {
    try {
        return primes && lsr::rns_moduli_for(n, primes) ? 0 : -1;
    } catch (...) {
        return -1;
    }
}

size_t lsr_ring_mod_capacity(uint64_t q, uint32_t n) noexcept {
    try {
        return lsr::ring_mod_capacity(q, n);
    } catch (...) {
        return 0;
    }
}

size_t lsr_ring_mod_capacity_bounded(uint64_t q, uint32_t n, uint64_t bound) noexcept {
    try {
        return lsr::ring_mod_capacity_bounded(q, n, bound);
    } catch (...) {
        return 0;
    }
}

LsrRingMod* lsr_ring_mod_create(uint64_t q, uint32_t n, int device) noexcept {
    const char* const where = "lsr_ring_mod_create";
    try {
        uint64_t p[2] = {0, 0};
        if (q < 2) return lsr::abi_refuse(where, "q = " + std::to_string(q) + ": the modulus must be at least 2"), nullptr;
        if (!lsr::rns_moduli_for(n, p))
            return lsr::abi_refuse(where, "n = " + std::to_string(n) + ": the ring degree must be a power of two in [2, 131072] with two 44-bit NTT primes"), nullptr;
        const size_t max_terms = lsr::ring_mod_capacity(q, n);
        if (max_terms == 0)
            return lsr::abi_refuse(where, "q = " + std::to_string(q) + " is too large at n = " + std::to_string(n) +
                                              ": one product needs n floor(q/2)^2 <= (p1 p2 - 1) / 2 (lsr_ring_mod_capacity)"),
                   nullptr;
        device = lsr::resolve_device(where, device, true);
        if (device < 0) return nullptr;
        std::unique_ptr<LsrRingMod> h(new LsrRingMod);
        lsr::DeviceGuard guard(device);
        h->q = q;
        h->n = n;
        h->device = device;
        h->max_terms = max_terms;
        for (int i = 0; i < 2; ++i) {
            h->prime[i].reset(lsr::create_ntt_context(p[i], n, device));
            if (!h->prime[i]) return lsr::abi_refuse(where, std::string("prime context: ") + lsr::last_error_cstr()), nullptr;
            h->lift[i] = lsr::LiftSource{q >> 1, p[i] - q};
        }
        h->logn = h->prime[0]->logn;
        h->coeff.reset(lsr::create_coeff_context(where, q, n, h->logn, device));
        if (!h->coeff) return nullptr;   // (create_coeff_context set lsr_last_error)
        h->pq = lsr::make_mod_params(q, h->logn);
        const lsr::u128 big = (lsr::u128)p[0] * p[1], half = (big - 1) / 2;
        h->rc.p[0] = p[0];
        h->rc.p[1] = p[1];
        h->rc.p1inv = lsr::invmod_prime(p[0] % p[1], p[1]);
        h->rc.half_lo = (uint64_t)half;
        h->rc.half_hi = (uint64_t)(half >> 64);
        h->rc.p1_mod_q = p[0] % q;
        h->rc.big_mod_q = (uint64_t)(big % q);
        if (h->logn <= lsr::kTileLog) {
            h->chunk = lsr::kRingModSumWords >> h->logn;
            h->bhat_rows = std::min<size_t>(lsr::kRingModBhatMaxRows, lsr::kRingModBhatWords >> h->logn);
            h->ws.allocate(2 * (h->chunk + h->bhat_rows) * n + lsr::kRingModFoldFlagWords);
        }
        return h.release();
    } catch (const std::exception& e) {
        lsr::set_last_error(std::string(where) + ": " + e.what());
        return nullptr;
    } catch (...) {
        return nullptr;
    }
}

void lsr_ring_mod_free(LsrRingMod* h) noexcept {
    if (!h) return;
    try {
        lsr::DeviceGuard guard(h->device);
        h->event.sync();             // a call still in flight uses the workspace and the prime contexts' tables
    } catch (...) {
    }
    delete h;
}

uint64_t lsr_ring_mod_modulus(const LsrRingMod* h) noexcept { return h ? h->q : 0; }
const NttContext* lsr_ring_mod_prime_context(const LsrRingMod* h, int i) noexcept { return h && (i == 0 || i == 1) ? h->prime[i].get() : nullptr; }
size_t lsr_ring_mod_max_terms(const LsrRingMod* h) noexcept { return h ? h->max_terms : 0; }
const NttContext* lsr_ring_mod_coeff_context(const LsrRingMod* h) noexcept { return h ? h->coeff.get() : nullptr; }

int lsr_ring_mod_lift_batch_device(const LsrRingMod* h, int i, uint64_t* d_out, const uint64_t* d_x, size_t count, void* stream) noexcept {
    const char* const where = "lsr_ring_mod_lift_batch_device";
    if (!h || !d_out || !d_x) return lsr::abi_refuse(where, "NULL handle or buffer");
    if (i != 0 && i != 1) return lsr::abi_refuse(where, "i = " + std::to_string(i) + ": the prime index must be 0 or 1");
    const int rc = stream_check(where, count);
    if (rc != 0) return rc < 0 ? -1 : 0;
    return lsr::abi_guarded(where, [&] {
        require_words({d_out, d_x});
        require_same_or_apart(d_out, d_x, count * 8, "d_out overlaps d_x in part: the output is the operand itself or apart from it");
        lsr::require_device();
        lsr::DeviceGuard guard(h->device);
        lsr::launch_lift(*h, i, d_out, d_x, count, static_cast<hipStream_t>(stream));
    });
}

int lsr_ring_mod_reduce_batch_device(const LsrRingMod* h, uint64_t* d_out, const uint64_t* d_r0, const uint64_t* d_r1, size_t count, int accumulate,
                                     void* stream) noexcept {
    const char* const where = "lsr_ring_mod_reduce_batch_device";
    if (!h || !d_out || !d_r0 || !d_r1) return lsr::abi_refuse(where, "NULL handle or buffer");
    const int rc = stream_check(where, count);
    if (rc != 0) return rc < 0 ? -1 : 0;
    return lsr::abi_guarded(where, [&] {
        require_words({d_out, d_r0, d_r1});
        require_same_or_apart(d_out, d_r0, count * 8, "d_out overlaps d_r0 in part: the output is an operand itself or apart from it");
        require_same_or_apart(d_out, d_r1, count * 8, "d_out overlaps d_r1 in part: the output is an operand itself or apart from it");
        lsr::require_device();
        lsr::DeviceGuard guard(h->device);
        lsr::launch_reduce(*h, d_out, d_r0, d_r1, count, accumulate != 0, static_cast<hipStream_t>(stream));
    });
}

int lsr_ring_mod_mul_batch(const LsrRingMod* h, uint64_t* c, const uint64_t* a, const uint64_t* b, size_t batch, size_t b_rows) noexcept {
    return ring_mod_dot_call("lsr_ring_mod_mul_batch", h, c, a, b, batch, 1, b_rows, true, false, nullptr);
}
int lsr_ring_mod_mul_batch_device(const LsrRingMod* h, uint64_t* d_c, const uint64_t* d_a, const uint64_t* d_b, size_t batch, size_t b_rows,
                                  void* stream) noexcept {
    return ring_mod_dot_call("lsr_ring_mod_mul_batch_device", h, d_c, d_a, d_b, batch, 1, b_rows, true, true, stream);
}
int lsr_ring_mod_dot_batch(const LsrRingMod* h, uint64_t* c, const uint64_t* a, const uint64_t* b, size_t batch, size_t terms, size_t b_rows) noexcept {
    return ring_mod_dot_call("lsr_ring_mod_dot_batch", h, c, a, b, batch, terms, b_rows, false, false, nullptr);
}
int lsr_ring_mod_dot_batch_device(const LsrRingMod* h, uint64_t* d_c, const uint64_t* d_a, const uint64_t* d_b, size_t batch, size_t terms, size_t b_rows,
                                  void* stream) noexcept {
    return ring_mod_dot_call("lsr_ring_mod_dot_batch_device", h, d_c, d_a, d_b, batch, terms, b_rows, false, true, stream);
}
int lsr_ring_mod_dot_galois_batch(const LsrRingMod* h, uint64_t* c, const uint64_t* a, const uint64_t* b, size_t batch, size_t terms, size_t b_rows,
                                  uint64_t g) noexcept {
    return ring_mod_dot_call("lsr_ring_mod_dot_galois_batch", h, c, a, b, batch, terms, b_rows, false, false, nullptr, true, g);
}
int lsr_ring_mod_dot_galois_batch_device(const LsrRingMod* h, uint64_t* d_c, const uint64_t* d_a, const uint64_t* d_b, size_t batch, size_t terms,
                                         size_t b_rows, uint64_t g, void* stream) noexcept {
    return ring_mod_dot_call("lsr_ring_mod_dot_galois_batch_device", h, d_c, d_a, d_b, batch, terms, b_rows, false, true, stream, true, g);
}

}  // extern "C"
