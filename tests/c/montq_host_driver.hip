// Stand-alone host driver for the __host__ __device__ arithmetic of the Lagrange prove path: lsr_montq.hpp (mq_*) and
// lsr_lagrange_kernels.hpp (Acc192, gv_*, verify_one_generic), each against unsigned __int128.  Built as the library is built
// (hipcc --offload-arch=gfx950) with UndefinedBehaviorSanitizer on the host pass and run as a plain program by
// tests/test_montq_host.py.  It makes no device call, so it needs no GPU.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lsr_lagrange_kernels.hpp"

using namespace lsr;
typedef unsigned __int128 u128;

static long g_checks = 0;
static const uint64_t kMax = ~(uint64_t)0;
#define CHECK(cond, ...)                                        \
    do {                                                        \
        ++g_checks;                                             \
        if (!(cond)) {                                          \
            std::printf("FAIL %s:%d: %s\n  ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                           \
            std::printf("\n");                                  \
            std::exit(1);                                       \
        }                                                       \
    } while (0)

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {   // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static uint64_t ref_mul(uint64_t a, uint64_t b, uint64_t q) { return (uint64_t)((u128)(a % q) * (b % q) % q); }
// arith.rs sub_mod in u128: (a + q - b) wrapping, one conditional subtraction, truncated
static uint64_t ref_sub_wrapping(uint64_t a, uint64_t b, uint64_t q) {
    u128 d = (u128)a + q - (u128)b;
    if (d >= q) d -= q;
    return (uint64_t)d;
}
static uint64_t ref_vanishing(uint64_t x, uint32_t m, uint64_t q) {
    uint64_t r = 1 % q;
    for (uint32_t i = 0; i < m; ++i) r = ref_mul(r, ref_sub_wrapping(x, (uint64_t)i % q, q), q);
    return r;
}
// verify_r1cs[_zk] after the two challenges are re-derived, on any 64-bit proof words
static int ref_verify(const uint64_t* p, uint64_t alpha, uint64_t beta, uint32_t m, bool zk, uint64_t q) {
    if (p[0] != alpha) return 0;
    if (p[1] != beta) return 0;
    for (int k = 0; k < 2; ++k) {
        const uint64_t zh = ref_vanishing(p[k], m, q);
        uint64_t qv = p[2 + k];
        if (zk) qv = ref_sub_wrapping(qv, ref_mul(p[12], zh, q), q);
        if (ref_mul(qv, zh, q) != ref_sub_wrapping(ref_mul(p[4 + 3 * k], p[5 + 3 * k], q), p[6 + 3 * k], q)) return 0;
    }
    return (p[10] == p[2] && p[11] == p[3]) ? 1 : 0;
}

// x 2^-64 r1 = x (mod q): `got` is the canonical x 2^-64 exactly when got < q and got r1 = x mod q (r1 is a unit)
static bool is_redc_of(uint64_t got, uint64_t x_mod_q, const MontQ& M) { return got < M.q && (uint64_t)((u128)got * M.r1 % M.q) == x_mod_q; }

static void check_constants(const MontQ& M) {
    const uint64_t q = M.q;
    CHECK((uint64_t)(q * M.qinv) == ~0ull, "q=%" PRIu64, q);
    u128 r = 1;
    for (int i = 0; i < 64; ++i) r = r * 2 % q;
    CHECK(M.r1 == (uint64_t)r, "q=%" PRIu64, q);
    CHECK(M.r2 == (uint64_t)(r * r % q) && M.r3 == (uint64_t)(r * r % q * r % q), "q=%" PRIu64, q);
}

static void check_pair(uint64_t a, uint64_t b, const MontQ& M) {
    const uint64_t q = M.q;
    if (a < q || b < q) CHECK(is_redc_of(mq_mul(a, b, M), ref_mul(a, b, q), M), "mq_mul q=%" PRIu64 " a=%" PRIu64 " b=%" PRIu64, q, a, b);
    if (a < q && b < q) {
        CHECK(mq_add(a, b, M) == (uint64_t)(((u128)a + b) % q), "mq_add q=%" PRIu64 " a=%" PRIu64 " b=%" PRIu64, q, a, b);
        CHECK(mq_sub(a, b, M) == (uint64_t)(((u128)a + q - b) % q), "mq_sub q=%" PRIu64 " a=%" PRIu64 " b=%" PRIu64, q, a, b);
    }
    if (a < q) {   // hi:lo < q 2^64
        const uint64_t x = (uint64_t)((((u128)(a % q) * M.r1) % q + b % q) % q);
        CHECK(is_redc_of(mq_redc(a, b, M), x, M), "mq_redc q=%" PRIu64 " hi=%" PRIu64 " lo=%" PRIu64, q, a, b);
    }
    CHECK(gv_mul(a, b, M) == ref_mul(a, b, q), "gv_mul q=%" PRIu64 " a=%" PRIu64 " b=%" PRIu64, q, a, b);
    CHECK(gv_sub(a, b, q) == ref_sub_wrapping(a, b, q), "gv_sub q=%" PRIu64 " a=%" PRIu64 " b=%" PRIu64, q, a, b);
    if (a < q && b < q) CHECK(gv_sub(a, b, q) == (uint64_t)(((u128)a + q - b) % q), "gv_sub canonical q=%" PRIu64, q);
}

static void check_word(uint64_t x, const MontQ& M) {
    const uint64_t q = M.q;
    CHECK(mq_to(x, M) == (uint64_t)((u128)(x % q) * M.r1 % q), "mq_to q=%" PRIu64 " x=%" PRIu64, q, x);
    CHECK(mq_canon(x, M) == x % q, "mq_canon q=%" PRIu64 " x=%" PRIu64, q, x);
    for (uint32_t m : {0u, 1u, 2u, 17u, 65u}) CHECK(gv_vanishing(x, m, M) == ref_vanishing(x, m, q), "gv_vanishing q=%" PRIu64 " x=%" PRIu64 " m=%u", q, x, m);
}

// acc_mac over the pairs against a 192-bit sum kept as (u128 low, carries), then acc_reduce against the sum mod q
static void check_sum(const std::vector<uint64_t>& x, const std::vector<uint64_t>& y, const MontQ& M, const char* what) {
    const uint64_t q = M.q;
    Acc192 acc;
    acc_zero(acc);
    u128 low = 0;
    uint64_t high = 0, mod = 0;
    for (size_t i = 0; i < x.size(); ++i) {
        acc_mac(acc, x[i], y[i]);
        const u128 p = (u128)x[i] * y[i];
        low += p;
        high += low < p ? 1u : 0u;
        mod = (uint64_t)(((u128)mod + ref_mul(x[i], y[i], q)) % q);
    }
    CHECK(acc.t0 == (uint64_t)low && acc.t1 == (uint64_t)(low >> 64) && acc.t2 == high, "acc_mac %s q=%" PRIu64 " terms=%zu", what, q, x.size());
    const uint64_t got = acc_reduce(acc, M);   // S 2^-128: two factors of r1 bring it back
    CHECK(got < q && (uint64_t)((u128)got * M.r2 % q) == mod, "acc_reduce %s q=%" PRIu64 " terms=%zu got=%" PRIu64, what, q, x.size(), got);
}

// S = q + j 2^128 for j < 8192: the second Montgomery step ends in q + j, past 2^64 once j >= 2^64 - q; the result is j mod q
static void check_carry_states(const MontQ& M) {
    const uint64_t q = M.q;
    for (uint64_t j : {(uint64_t)0, (uint64_t)1, (uint64_t)58, (uint64_t)59, (uint64_t)60, (uint64_t)4096, (uint64_t)8191}) {
        Acc192 acc{q, 0, j};
        if (j >= (uint64_t)(((u128)q * q) >> 115)) continue;   // S >= 2^13 q^2: outside acc_reduce's contract
        CHECK(acc_reduce(acc, M) == j % q, "acc_reduce carry state q=%" PRIu64 " j=%" PRIu64, q, j);
    }
}

static void check_verify(const MontQ& M) {
    const uint64_t q = M.q;
    const uint64_t edge[] = {0, 1, q - 2, q - 1, q, kMax};
    for (uint32_t m : {1u, 2u, 17u, 65u})
        for (int zk = 0; zk < 2; ++zk)
            for (int round = 0; round < 40; ++round) {
                // a proof that verifies: Q'(x) Z_H(x) = A B - C at both points, for any words in the remaining slots
                uint64_t p[13];
                for (int k = 0; k < 2; ++k) {
                    p[k] = round < 6 ? edge[round] % q : rnd() % q;
                    const uint64_t zh = ref_vanishing(p[k], m, q);
                    const uint64_t r = rnd() % q, qv = rnd() % q;
                    p[12] = k == 0 ? r : p[12];
                    const uint64_t qprime = zk ? (uint64_t)(((u128)qv + ref_mul(p[12], zh, q)) % q) : qv;
                    p[2 + k] = qprime;
                    p[4 + 3 * k] = rnd() % q;
                    p[5 + 3 * k] = rnd() % q;
                    p[6 + 3 * k] = (uint64_t)(((u128)ref_mul(p[4 + 3 * k], p[5 + 3 * k], q) + q - ref_mul(qv, zh, q)) % q);
                    p[10 + k] = p[2 + k];
                }
                if (!zk) p[12] = 0;
                CHECK(ref_verify(p, p[0], p[1], m, zk, q) == 1, "reference rejects its own proof q=%" PRIu64, q);
                CHECK(verify_one_generic(p, p[0], p[1], m, zk, M) == 1, "verify_one_generic rejects q=%" PRIu64 " m=%u zk=%d", q, m, zk);
                CHECK(verify_one_generic(p, p[0] ^ 1, p[1], m, zk, M) == 0 && verify_one_generic(p, p[0], p[1] ^ 1, m, zk, M) == 0, "challenge q=%" PRIu64, q);
                for (int w = 0; w < 13; ++w)
                    for (uint64_t val : {p[w] ^ 2, q, kMax, p[w] + q, rnd()}) {
                        uint64_t t[13];
                        for (int i = 0; i < 13; ++i) t[i] = p[i];
                        t[w] = val;
                        CHECK(verify_one_generic(t, p[0], p[1], m, zk, M) == ref_verify(t, p[0], p[1], m, zk, q),
                              "verify_one_generic q=%" PRIu64 " m=%u zk=%d word=%d val=%" PRIu64, q, m, zk, w, val);
                    }
            }
}

static void run_modulus(uint64_t q) {
    const MontQ M = make_mont(q);
    check_constants(M);
    std::vector<uint64_t> words;
    if (q <= 7) {
        for (uint64_t a = 0; a < q; ++a) words.push_back(a);            // every canonical pair
        for (uint64_t x : {q, q + 1, 2 * q, kMax, kMax - 1}) words.push_back(x);
    } else {
        for (uint64_t x : {(uint64_t)0, (uint64_t)1, q - 2, q - 1, q, kMax}) words.push_back(x);
        for (int i = 0; i < 40; ++i) words.push_back(rnd());
        for (int i = 0; i < 40; ++i) words.push_back(rnd() % q);
        for (int i = 0; i < 8; ++i) words.push_back(q - 1 - (rnd() & 0xFF));
    }
    for (uint64_t a : words) {
        check_word(a, M);
        for (uint64_t b : words) check_pair(a, b, M);
    }
    for (size_t n : {(size_t)1, (size_t)2, (size_t)17, (size_t)100, (size_t)1024, (size_t)8192}) {
        std::vector<uint64_t> x(n, q - 1), y(n, q - 1);
        check_sum(x, y, M, "all (q-1)^2");
        for (auto& v : y) v = rnd() % q;
        check_sum(x, y, M, "(q-1) random");
        for (auto& v : x) v = rnd() % q;
        check_sum(x, y, M, "random random");
        x.assign(n, 0);
        y.assign(n, 0);
        const size_t at = rnd() % n;
        x[at] = y[at] = q - 1;
        check_sum(x, y, M, "spike");
        y[at] = 1;
        check_sum(x, y, M, "spike times one");
    }
    check_carry_states(M);
    check_verify(M);
}

int main() {
    const uint64_t moduli[] = {3, 5, 7, 16381, 16411, 32749, (1ull << 32) - 1, (1ull << 32) + 1, (1ull << 63) - 1, (1ull << 63) + 1,
                               9223372036854775837ull,                      // the first prime above 2^63
                               4294967291ull * 4294967279ull,               // composite above 2^63
                               0xFFFFFFFF00000001ull,                       // Goldilocks
                               18446744073709551557ull,                     // 2^64 - 59
                               ~0ull};
    for (uint64_t q : moduli) run_modulus(q);
    std::printf("ok: %zu moduli, %ld checks\n", sizeof(moduli) / sizeof(moduli[0]), g_checks);
    return 0;
}
