"""Model of the resident-matrix products under an arbitrary modulus (lsr_ring_mod_matrix_* / lsr_ring_mod_matvec_*, batch.h, DESIGN.md
§5q) in Python integers, on top of ring_mod_model (the negacyclic inner product mod q), ring_gadget_model (the digits, taken against
q) and ring_sample_model (the UNIFORM element with modulus q).  Independent of the library: no grouping, no primes in the products."""
import numpy as np

import ring_gadget_model as gadget
import ring_mod_model as mod
import ring_sample_model as sample


def matvec(m, x, q):
    """m [rows][cols][n], x [batch][cols][n] -> y [batch][rows][n] uint64: y[j][r] = sum_c m[r][c] x[j][c] mod (X^n + 1, q)"""
    m, x = np.asarray(m, dtype=np.uint64), np.asarray(x, dtype=np.uint64)
    rows = [row.tolist() for row in m]
    return np.array([[mod.negacyclic_dot(row, xj, q) for row in rows] for xj in x.tolist()], dtype=np.uint64)


def matvec_coefficient(m, x, q, j, r, k):
    """coefficient k of y[j][r]"""
    return mod.dot_coefficient(np.asarray(m)[r].tolist(), np.asarray(x)[j].tolist(), q, k)


def decomposed(x, q, b, digits):
    """x [batch][xcols][n] -> G^-1(x) [batch][xcols digits][n], the digits taken against q, as canonical residues mod q"""
    return gadget.gadget_inverse(np.asarray(x, dtype=np.uint64), q, b, digits)


def matvec_gadget(m, x, q, b, digits):
    assert gadget.admissible(q, b, digits)
    return matvec(m, decomposed(x, q, b, digits), q)


def capacity_bounded(q, n, bound):
    """floor(((P - 1) / 2) / (n h bound)), h = floor(q / 2), saturated at 2^64 - 1; 0: bound outside [1, h] or capacity(q, n) == 0"""
    if mod.capacity(q, n) == 0 or bound == 0 or bound > q // 2:
        return 0
    p1, p2 = mod.primes(n)
    return min((p1 * p2 - 1) // 2 // (n * (q // 2) * bound), 2**64 - 1)


def seeded_matrix(oracle, q, n, key, domain, index_base, rows, cols):
    """[rows][cols][n]: entry [r][c] the UNIFORM element with modulus q of stream index index_base + r cols + c under `key`"""
    words, _ = sample.sample(oracle, q, n, rows * cols, sample.UNIFORM, 0, [key], rows * cols, domain=domain, index_base=index_base)
    return words.reshape(rows, cols, n)


# ---- the model's own tests (collected through tests/test_ring_mod_matvec_abi.py) ---------------------------------------------------
def test_model_matvec_is_the_schoolbook_and_the_gadget_recomposes():
    rng = np.random.default_rng(3)
    for n, q, b in [(4, 3329, 4), (8, (1 << 40) + 15, 8), (4, 1 << 32, 11)]:
        m = rng.integers(0, q, size=(2, 3, n), dtype=np.uint64)
        x = rng.integers(0, q, size=(2, 3, n), dtype=np.uint64)
        want = [[[0] * n for _ in range(2)] for _ in range(2)]
        for j in range(2):
            for r in range(2):
                for c in range(3):
                    prod = mod.negacyclic_mul_schoolbook(m[r, c].tolist(), x[j, c].tolist(), q)
                    want[j][r] = [(u + v) % q for u, v in zip(want[j][r], prod)]
        assert matvec(m, x, q).tolist() == want
        assert matvec_coefficient(m, x, q, 1, 0, n - 1) == want[1][0][n - 1]
        digits = gadget.min_digits(q, b)
        z = decomposed(x, q, b, digits)
        assert z.shape == (2, 3 * digits, n)
        assert np.array_equal(gadget.recompose(z.reshape(2, 3, digits, n), q, b), x)          # G G^-1 = id
        centred = [mod.centre(int(v), q) for v in z.reshape(-1)]
        assert max(centred) <= (1 << (b - 1)) - 1 and min(centred) >= -(1 << (b - 1))


def test_model_capacity_bounded():
    q, n = (1 << 40) + 15, 64
    assert capacity_bounded(q, n, q // 2) == mod.capacity(q, n) == 7
    assert capacity_bounded(q, n, 1 << 31) == 2047 and capacity_bounded(q, n, 128) == 34359705185      # b = 8: 3.4 10^10 against 7
    assert capacity_bounded(q, n, 0) == 0 == capacity_bounded(q, n, q // 2 + 1)
    assert capacity_bounded(2, 64, 1) == 2**64 - 1 and capacity_bounded(3329, 3, 1) == 0
