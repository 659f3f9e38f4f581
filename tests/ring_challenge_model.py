"""Python-integer model of the fixed-point operator norm and of the operator-norm-bounded challenge sampler (batch.h
"operator-norm-bounded ring challenges"), on top of ring_sample_model's streams and its rejection primitive draw.
TEST INFRASTRUCTURE.

  * table(n):        C[j] = round(2^30 cos(pi j / n)) from math.cos;
  * opnorm(c, ...):  N(c) = max over e in E of Re_e^2 + Im_e^2 — the sums in numpy int64 (they fit: the caller keeps |c_i| <= 2^15),
                     the squares in Python integers;
  * challenge(...):  the attempt loop, with per-element statistics: the tries, and the draws that went past word 0.
The tests at the bottom (no GPU) pin N on elements whose norm is known and compare it with numpy's FFT."""
import math

import numpy as np

from ring_sample_model import Stats, Stream, draw

ATTEMPT_WORDS = 1 << 18
MAX_TRIES = 1024
MAX_DEGREE = 4096
MAX_COEFFICIENT = 1 << 15
ALL_ONES = (1 << 128) - 1
SCALE = 1 << 30

_TABLES = {}


def table(n):
    """C[j] = round(2^30 cos(pi j / n)), 0 <= j < 2n, as a numpy int64 array (no entry is near a tie: floor(x + 1/2) is the rounding)."""
    assert 2 <= n <= MAX_DEGREE and n & (n - 1) == 0
    if n not in _TABLES:
        _TABLES[n] = np.array([math.floor(SCALE * math.cos(math.pi * j / n) + 0.5) for j in range(2 * n)], dtype=np.int64)
    return _TABLES[n]


def exponents(n, cyclic):
    """E: one exponent per conjugate pair of the ring's complex embeddings."""
    return [2 * k for k in range(n // 2 + 1)] if cyclic else [2 * k + 1 for k in range(n // 2)]


def centred(words, q):
    return [w - q if w > q // 2 else w for w in (int(w) for w in words)]


def opnorm_centred(coefficients, n, cyclic):
    """N(c) of centred coefficients (|c_i| <= 2^15) as a Python int."""
    assert len(coefficients) == n
    positions = np.array([i for i, c in enumerate(coefficients) if c], dtype=np.int64)
    values = np.array([c for c in coefficients if c], dtype=np.int64)
    if positions.size == 0:
        return 0
    assert int(np.abs(values).max()) <= MAX_COEFFICIENT
    tab, e = table(n), np.array(exponents(n, cyclic), dtype=np.int64)
    at = (e[:, None] * positions[None, :]) % (2 * n)
    re = tab[at] @ values
    im = tab[(at - n // 2) % (2 * n)] @ values
    return max(int(r) * int(r) + int(i) * int(i) for r, i in zip(re.tolist(), im.tolist()))


def opnorm(words, q, cyclic=False):
    """N(c) of one element of canonical words, or 2^128 - 1 for a word >= q or a centred coefficient above 2^15 in magnitude."""
    words = [int(w) for w in words]
    if any(w >= q for w in words):
        return ALL_ONES
    c = centred(words, q)
    if any(abs(v) > MAX_COEFFICIENT for v in c):
        return ALL_ONES
    return opnorm_centred(c, len(words), cyclic)


def bound_of(t):
    """T^2 2^60: "norm <= T" means N(c) <= bound_of(T)."""
    return t * t << 60


def candidate(stream, n, kappa1, kappa2, attempt, stats):
    """The centred coefficients of attempt `attempt`: BALL's inside-out shuffle at word offset attempt 2^18, magnitude 2 for the first
    kappa2 steps."""
    kappa, base = kappa1 + kappa2, attempt * ATTEMPT_WORDS
    first = [int(w) for w in stream.words(base, kappa)]
    c = [0] * n
    for s in range(kappa):
        i = n - kappa + s
        j = draw(i + 1, lambda a, s=s: first[s] if a == 0 else stream.word(base + a * kappa + s), 63, stats)
        c[i] = c[j]
        c[j] = (2 if s < kappa2 else 1) * (-1 if first[s] >> 63 else 1)
    return c


class ChallengeStats:
    """Of one element: tries (0: exhausted), the norm of every candidate looked at, and the draws of all its attempts (Stats)."""

    def __init__(self):
        self.tries, self.norms, self.draws = 0, [], Stats()


def challenge(oracle, q, n, count, kappa1, kappa2, opnorm_bound, max_tries, keys, components, domain=16, index_base=0, cyclic=False):
    """-> ([count, n] uint64, int32 [count] tries, [ChallengeStats per element])"""
    assert components >= 1 and len(keys) >= -(-count // components)
    assert 1 <= kappa1 + kappa2 <= n <= MAX_DEGREE and (kappa2 == 0 or q >= 5) and 1 <= max_tries <= MAX_TRIES and 0 <= opnorm_bound < 1 << 32
    out, tries, stats = np.zeros((count, n), dtype=np.uint64), np.zeros(count, dtype=np.int32), []
    limit = bound_of(opnorm_bound)
    for e in range(count):
        stream = Stream(oracle, keys[e // components], domain, index_base + e % components)
        st = ChallengeStats()
        for t in range(max_tries):
            c = candidate(stream, n, kappa1, kappa2, t, st.draws)
            if opnorm_bound:
                st.norms.append(opnorm_centred(c, n, cyclic))
            if not opnorm_bound or st.norms[-1] <= limit:
                st.tries = t + 1
                out[e] = np.array([v % q for v in c], dtype=np.uint64)
                break
        tries[e] = st.tries
        stats.append(st)
    return out, tries, stats


def float_norm(coefficients, n, cyclic):
    """The operator norm in floating point: the largest |c(zeta)| over the roots of X^n + 1 (cyclic: X^n - 1), by numpy's FFT of the
    twisted coefficients."""
    c = np.array(coefficients, dtype=np.float64)
    if not cyclic:
        c = c * np.exp(1j * np.pi * np.arange(n) / n)
    return float(np.abs(np.fft.fft(c)).max())


# ---- the model's own tests (collected by test_ring_challenge_abi.py) ------------------------------------------------------------------
def _documented_error(coefficients):
    """sqrt(2) ||c||_1 2^-31: every table entry is off by at most 1/2 in units of 2^-30, in Re and in Im."""
    return math.sqrt(2) * sum(abs(v) for v in coefficients) / 2**31


def test_norm_of_one_is_exactly_one():
    for n in (2, 4, 64, 4096):
        for cyclic in (False, True):
            assert opnorm_centred([1] + [0] * (n - 1), n, cyclic) == 1 << 60
            assert opnorm([1] + [0] * (n - 1), 12289, cyclic) == 1 << 60


def test_norm_of_a_monomial_is_one_within_the_documented_error():
    for n in (2, 8, 64, 1024):
        for i in range(n):
            c = [0] * n
            c[i] = -1 if i % 3 == 0 else 1
            for cyclic in (False, True):
                assert abs(math.sqrt(opnorm_centred(c, n, cyclic)) / SCALE - 1) <= _documented_error(c), (n, i, cyclic)


def test_cyclic_all_ones_has_norm_n_reached_at_e_zero():
    for n in (2, 8, 64, 4096):
        assert opnorm_centred([1] * n, n, True) == n * n << 60
        assert opnorm([1] * n, 12289, True) == n * n << 60


def test_norm_agrees_with_the_fft_norm_on_random_inputs():
    rng = np.random.default_rng(30)
    for n in (2, 4, 16, 64, 256, 4096):
        for cyclic in (False, True):
            for bound in (1, 2, MAX_COEFFICIENT):
                c = [int(v) for v in rng.integers(-bound, bound + 1, size=n)]
                if not any(c):
                    c[0] = 1
                mine, ref = math.sqrt(opnorm_centred(c, n, cyclic)) / SCALE, float_norm(c, n, cyclic)
                assert abs(mine - ref) <= 1e-6 * ref, (n, cyclic, bound)
                assert abs(mine - ref) <= _documented_error(c) + 1e-9 * ref      # (the FFT's own rounding)


def test_out_of_range_elements_are_all_ones():
    q = 12289
    assert opnorm([0, q, 0, 0], q) == ALL_ONES and opnorm([0, q - 1, 0, 0], q) != ALL_ONES
    big = (1 << 61) - 1
    assert opnorm([MAX_COEFFICIENT + 1, 0], big) == ALL_ONES and opnorm([big - MAX_COEFFICIENT - 1, 0], big) == ALL_ONES
    assert opnorm([MAX_COEFFICIENT, big - MAX_COEFFICIENT], big) != ALL_ONES
