"""Test helper for tests/test_lagrange_tiles_gpu.py: directed inputs for the Lagrange (baseline) prove path and a
second, matrix-free reference for its interpolation.  The selector circuit turns the three constraint-evaluation vectors into free
inputs; `interpolant_at` evaluates an interpolant in O(m) Python-integer operations from the barycentric weights of {0..m-1} and
shares nothing with the matrix L of tests/lagrange_oracle.py or of the library; `steered` and `carry_instance` are satisfied
instances whose interpolants carry the largest sums the 192-bit accumulator meets.  The unmarked tests at the end pin the helper to
the oracle on the CPU.  Test infrastructure only — nothing here ships."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lagrange_oracle as lo  # noqa: E402

Q64 = (1 << 64) - 59                     # prime
QC = 4294967291 * 4294967279             # composite above 2^63, both factors prime
Q63 = 9223372036854775837                # the first prime above 2^63
assert QC == 18446743979220271189 and Q64 == 18446744073709551557


def selector_circuit(m):
    """n = 3m variables, A picks z[i], B picks z[m + i], C picks z[2m + i]: (A z, B z, C z) are the three thirds of the witness."""
    return 3 * m, [(i, i, 1) for i in range(m)], [(i, m + i, 1) for i in range(m)], [(i, 2 * m + i, 1) for i in range(m)]


def selector_witness(a, b, c):
    return np.array([int(v) for v in a] + [int(v) for v in b] + [int(v) for v in c], dtype=np.uint64)


def interpolant_at(evals, x, q):
    """P(x) for the P of degree < m with P(i) = evals[i] on {0..m-1}: sum_i e_i w_i prod_{j != i} (x - j) with
    w_i = 1 / (i! (m-1-i)! (-1)^(m-1-i)).  Needs (m-1)! to be a unit mod q."""
    m = len(evals)
    fact = [1] * m
    for i in range(1, m):
        fact[i] = fact[i - 1] * i % q
    inv_fact = [0] * m
    inv_fact[m - 1] = pow(fact[m - 1], -1, q)
    for i in range(m - 1, 0, -1):
        inv_fact[i - 1] = inv_fact[i] * i % q
    prefix = [1] * (m + 1)                # prefix[i] = prod_{j < i} (x - j)
    for j in range(m):
        prefix[j + 1] = prefix[j] * (x - j) % q
    suffix = [1] * (m + 1)                # suffix[i] = prod_{j >= i} (x - j)
    for j in range(m - 1, -1, -1):
        suffix[j] = suffix[j + 1] * (x - j) % q
    total = 0
    for i in range(m):
        term = int(evals[i]) % q * inv_fact[i] % q * inv_fact[m - 1 - i] % q * prefix[i] % q * suffix[i + 1] % q
        total += -term if (m - 1 - i) & 1 else term
    return total % q


def evaluate_on_domain(coeffs, q):
    """[P(0), ..., P(m-1)] for the m coefficients of P, by Horner"""
    return [lo.eval_poly(coeffs, i, q) for i in range(len(coeffs))]


def steered(m, q):
    """(a, b, c) with a_i = P(i) for the P whose m coefficients are all q - 1, b = a, c = a b: a satisfied instance whose
    interpolants A and B are all q - 1, so every product the quotient sums is (q - 1)^2."""
    a = []
    for i in range(m):
        if i == 0:
            s = 1
        elif i == 1:
            s = m
        else:
            try:
                s = (pow(i, m, q) - 1) * pow(i - 1, -1, q)          # 1 + i + ... + i^(m-1)
            except ValueError:
                s = lo.eval_poly([1] * m, i, q)
        a.append((q - 1) * s % q)
    return a, list(a), [v * v % q for v in a]


def carry_instance(m, q):
    """(a, b, c) = evaluations of polynomials A, B (and their pointwise product) chosen so that the first top coefficient of A B,
    S = sum_{s=1}^{m-1} A_s B_{m-s}, is exactly q + (m - 3) 2^128 as an integer.  The two Montgomery steps of S then end in
    V = (S + q (2^128 - 1)) / 2^128 = q + m - 3, which passes 2^64 when q > 2^64 - (m - 3): the one sum whose reduction leaves a carry
    out of 64 bits.  A_1 B_{m-1} = A_1 and A_2 B_{m-2} = A_2 (q - 1) are the two digits of what the other m - 3 products (q - 1)^2
    leave to S."""
    assert m >= 4
    rest = q + (m - 3) * (1 << 128) - (m - 3) * (q - 1) ** 2
    assert 0 <= rest < q * (q - 1)
    A = [q - 1] * m
    B = [q - 1] * m
    A[2], A[1] = divmod(rest, q - 1)
    B[m - 1] = 1
    assert sum(A[s] * B[m - s] for s in range(1, m)) == q + (m - 3) * (1 << 128)
    a, b = evaluate_on_domain(A, q), evaluate_on_domain(B, q)
    return (a, b, [x * y % q for x, y in zip(a, b)]), (A, B)


# ---- CPU self-tests ----------------------------------------------------------------------------------------------------------
SELF_MODULI = [Q64, QC, 16381]


@pytest.mark.parametrize("q", SELF_MODULI)
@pytest.mark.parametrize("m", [1, 2, 65, 129])
def test_interpolant_at_equals_the_oracle(m, q):
    rng = np.random.default_rng(m + q % 1009)
    e = [int(v) % q for v in rng.integers(0, 2**64, size=m, dtype=np.uint64)]
    if m > 2:
        e[0], e[m - 1] = q - 1, 0
    coeffs = lo.interpolate(e, q)
    for x in [0, 1, m - 1, m, q - 1] + [int(v) % q for v in rng.integers(0, 2**64, size=3, dtype=np.uint64)]:
        assert interpolant_at(e, x % q, q) == lo.eval_poly(coeffs, x % q, q), x
    for i in range(m):                                             # on the domain the interpolant returns its data
        assert interpolant_at(e, i, q) == e[i]


@pytest.mark.parametrize("q", SELF_MODULI + [Q63, 32749, 16411])
@pytest.mark.parametrize("m", [1, 2, 17, 65, 129])
def test_steered_is_all_q_minus_one_and_satisfied(m, q):
    a, b, c = steered(m, q)
    assert a == [(q - 1) * sum(pow(i, k, q) for k in range(m)) % q for i in range(m)]
    assert b == a and c == [x * x % q for x in a]
    assert lo.interpolate(a, q) == [q - 1] * m
    quot = lo.quotient((a, b, c), q)
    assert quot is not None and 1 <= len(quot) <= max(1, m - 1)


@pytest.mark.parametrize("m", [64, 65])
def test_carry_instance_sum_and_quotient(m):
    (a, b, c), (A, B) = carry_instance(m, Q64)
    assert lo.interpolate_many([a, b], Q64) == [A, B]
    S = sum(A[s] * B[m - s] for s in range(1, m))
    assert S % (1 << 128) == Q64 and (S + Q64 * ((1 << 128) - 1)) >> 128 == Q64 + m - 3 >= 1 << 64
    assert lo.quotient((a, b, c), Q64) is not None


@pytest.mark.parametrize("q", [97, Q64])
@pytest.mark.parametrize("m", [1, 5, 65])
def test_selector_circuit_reproduces_its_vectors(m, q):
    rng = np.random.default_rng(m)
    vecs = [[int(v) % q for v in rng.integers(0, 2**64, size=m, dtype=np.uint64)] for _ in range(3)]
    n, a, b, c = selector_circuit(m)
    z = selector_witness(*vecs)
    assert n == 3 * m == len(z)
    assert [lo.mat_vec(e, m, z, q) for e in (a, b, c)] == vecs
