// Host-side number theory and table construction for the MI355X commitment kernel.
// Product code (not the oracle).  Semantics follow SEAL 4.1's NTTTables / numth as used by the
// reference (cpp-core/src/ntt.cpp:46-59) — see SURVEY.md §8(a) row N2.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace lsr {

using u128 = unsigned __int128;

inline uint64_t mulmod(uint64_t a, uint64_t b, uint64_t q) { return (uint64_t)(((u128)a * b) % q); }
uint64_t powmod(uint64_t a, uint64_t e, uint64_t q);
inline uint64_t invmod_prime(uint64_t a, uint64_t q) { return powmod(a, q - 2, q); }
bool is_prime_u64(uint64_t n);
inline uint32_t bit_reverse(uint32_t x, int bits) {
    uint32_t r = 0;
    for (int i = 0; i < bits; ++i) { r = (r << 1) | (x & 1u); x >>= 1; }
    return r;
}

// Numerically smallest primitive (2n)-th root of unity mod prime q; 0 if q != 1 (mod 2n).
uint64_t minimal_primitive_root_2n(uint64_t q, uint32_t n);
// Largest prime p < 2^bits with p == 1 (mod factor); 0 if none above 2^(bits-1).
uint64_t largest_prime_congruent_one(uint64_t factor, int bits);

// Validation of (q, n) exactly as ntt_context_create must behave (ntt.cpp:30-70 + SEAL ctor rules).
bool ntt_params_valid(uint64_t q, uint32_t n, int* logn_out);

// Twiddle tables in "stage order": entry [m + i] (m = 2^s, i < m) is the twiddle of butterfly group i
// of the stage with m groups — forward: psi^bitrev(m+i); inverse: its modular inverse.  Entry [0] = 1.
struct TwiddleTables {
    std::vector<uint64_t> fwd;   // [n]
    std::vector<uint64_t> inv;   // [n]
    uint64_t psi = 0;
    uint64_t n_inv = 0;
};
TwiddleTables build_twiddles(uint64_t q, uint32_t n, int logn, uint64_t psi);

// Cyclic transform of the prover's polynomial path (rust-api/lambda-snark/src/ntt.rs:117-201): same butterfly network,
// other twiddles.  Entry [m + i] = omega^((n/2m) * bitrev_{log m}(i)) — group i of the m-group stage reduces modulo
// X^(n/m) - omega^((n/m) * bitrev(i)), so its twiddle is the square root of that constant; inverse table = inverses.
// Output of the forward network is f(omega^bitrev(i)) at slot i.
constexpr uint64_t kProverModulus = 0xFFFFFFFF00000001ull;       // NTT_MODULUS, lambda-snark-core/src/lib.rs:58
constexpr uint64_t kProverRoot2_32 = 1753635133440165772ull;     // NTT_PRIMITIVE_ROOT, lib.rs:78
// Montgomery form w 2^64 mod NTT_MODULUS of a residue: how the Goldilocks kernels hold their multipliers (gold_mul_mont)
inline uint64_t prover_montgomery(uint64_t w) { return mulmod(w % kProverModulus, 0xFFFFFFFFull, kProverModulus); }   // 2^64 = 2^32 - 1
// Size ceilings of the cyclic transforms and of everything built on them (quotient plan, R1CS prover): the entry points of the first
// five rounds stop at 2^17 (one strided round in front of the tile pass), the *_large constructors and the R1CS prover at 2^22 (two
// strided rounds; NTT_MODULUS only above 2^17).  lsr_prover_max_log2_size() reports the second.
constexpr int kTwoPassMaxLog2 = 17;
constexpr int kProverMaxLog2 = 22;
// n = 2^k in [2, 2^max_log2], prime q (q = NTT_MODULUS or q < 2^61), omega of exact order n.
bool cyclic_params_valid(uint64_t q, uint32_t n, uint64_t omega, int* logn_out, int max_log2 = kTwoPassMaxLog2);
// omega_n of compute_root_of_unity (ntt.rs:226-233); 0 unless q = NTT_MODULUS
uint64_t prover_root_of_unity(uint64_t q, uint64_t n);
TwiddleTables build_cyclic_twiddles(uint64_t q, uint32_t n, int logn, uint64_t omega);

// Shoup quotient floor(w * 2^64 / q)
inline uint64_t shoup_quotient(uint64_t w, uint64_t q) { return (uint64_t)(((u128)w << 64) / q); }

// CDT table of the reference sampler (cpp-core/src/utils.cpp:26-75). Empty on invalid sigma.
std::vector<uint64_t> gaussian_cdf(double sigma);
// Entries of `cdf` a scan at 63-bit precision has to visit: everything from the first entry whose upper 63 bits are all ones on
// can never be below a 63-bit uniform value, so `count += (cdf[k] >> 1 < u)` stops changing there (sigma = 3.19: 30 of 40).  The
// scan loops over k + 1 < entries, hence first saturated index + 1.  Same samples, bit for bit.
uint32_t gaussian_scan_entries(const std::vector<uint64_t>& cdf);

// Commitment parameter selection (DESIGN.md "Commitment definition").
uint64_t select_commit_modulus(uint64_t requested, uint32_t n);
uint64_t plain_modulus_for(uint32_t n);
// The two 44-bit NTT primes of ring degree n, shared by the RNS commitment contexts (lsr_commit.hip) and the ring
// handles of an arbitrary modulus (lsr_ring_mod.hip, §5p): out[0] = what a default commitment context picks, out[1] = the largest
// 44-bit prime = 1 (mod 2n) other than out[0]; both in (2^43, 2^44).  false: n is no power of two in [2, 131072] or there is no second prime.
bool rns_moduli_for(uint32_t n, uint64_t out[2]);
// How many products of ring elements mod q, degree n, may be summed and still be recovered from residues mod the two primes above
// (P = p1 p2): floor(((P - 1) / 2) / (n h^2)) with h = floor(q / 2), saturated at SIZE_MAX.  0: (q, n) is not admissible — q < 2, n
// not a power of two in [2, 131072], no prime pair, or not even one product fits.
size_t ring_mod_capacity(uint64_t q, uint32_t n);
// The same count when one operand of every product is short, its centred magnitude at most `bound` (the digits of a gadget
// decomposition: bound = B / 2; §5q): floor(((P - 1) / 2) / (n h bound)).  0 for bound == 0, for bound > h and wherever
// ring_mod_capacity is 0; ring_mod_capacity_bounded(q, n, h) == ring_mod_capacity(q, n).
size_t ring_mod_capacity_bounded(uint64_t q, uint32_t n, uint64_t bound);
// The same count when BOTH operands of every product are short (the Gram matrices of bounded ring vectors, §5r):
// floor(((P - 1) / 2) / (n bound_a bound_b)).  0 where a bound is 0 or above h and wherever ring_mod_capacity is 0;
// ring_mod_capacity_product(q, n, h, b) == ring_mod_capacity_bounded(q, n, b), ring_mod_capacity_product(q, n, h, h) == ring_mod_capacity(q, n).
size_t ring_mod_capacity_product(uint64_t q, uint32_t n, uint64_t bound_a, uint64_t bound_b);
// Triple negacyclic products g c c' with |g| <= bound_g and |c|, |c'| <= bound_c that one sum may hold:
// floor(((P - 1) / 2) / (n^2 bound_g bound_c^2)), the divisions taken one after the other (the divisor can exceed 128 bits).  A bound
// of 0 states none: h.  0 where a bound is above h and wherever ring_mod_capacity is 0; saturated at SIZE_MAX.
size_t ring_mod_capacity_quadform(uint64_t q, uint32_t n, uint64_t bound_g, uint64_t bound_c);

uint64_t os_entropy64();

}  // namespace lsr
