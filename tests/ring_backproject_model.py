"""Python-integer model of the adjoint Pi^T w of the seeded Johnson-Lindenstrauss projection (lsr_ntt_ring_project_adjoint_batch,
batch.h "norms and projections of ring vectors").  TEST INFRASTRUCTURE.  The matrix entries come from
``ring_norm_model.matrix_signs`` (the CPU oracle's stream words), the conjugation from ``ring_galois_model.automorphism_np``.

Exactness at 64-bit moduli: a weight w < 2^64 is split as w = h 2^32 + l; sum_r h_r pi[r][pos] and sum_r l_r pi[r][pos] are sums of
256 terms below 2^32 in absolute value, so numpy's int64 holds them exactly (|sum| < 2^40); they are put together and reduced mod q in
Python integers.  ``back_project_ints`` is the same sum term by term in Python integers; the model's own tests hold the two against
each other with every weight q - 1 at the 60-bit prime and at Goldilocks."""
import numpy as np

import ring_galois_model as galois
import ring_norm_model as norm
from ring_norm_model import ROWS, key_from_bytes, key_from_seed  # noqa: F401  (re-exported for the tests)
from ring_sample_model import Stream

MAX_SETS = 16
Q60 = 1152921504606584833
GOLD = 2**64 - 2**32 + 1
_SIGNS = {}


def signs_of(oracle, length, key, domain, index):
    """[256, length] int8 of the matrix whose row r is the stream (key, domain, index + r); short matrices are kept for the next call."""
    who = (tuple(int(k) for k in key), int(domain), int(index), int(length))
    if who in _SIGNS:
        return _SIGNS[who]
    signs = norm.matrix_signs(oracle, length, key, domain, index)
    if length <= 1 << 14:
        _SIGNS[who] = signs
    return signs


def weighted_columns(signs, weights, q):
    """signs [256, length] in {-1, 0, 1}, weights [sets][256] integers below 2^64 -> [sets, length] uint64:
    sum_r weights[k][r] signs[r][pos] mod q."""
    w = [[int(v) for v in row] for row in weights]
    assert all(len(row) == ROWS and all(0 <= v < 2**64 for v in row) for row in w)
    halves = np.array([[v >> 32 for v in row] for row in w] + [[v & 0xFFFFFFFF for v in row] for row in w], dtype=np.int64)
    sums = np.zeros((len(halves), signs.shape[1]), dtype=np.int64)
    for r in range(0, ROWS, 32):                                  # 32 rows at a time: the int64 copy of the signs stays small
        sums += halves[:, r:r + 32] @ signs[r:r + 32].astype(np.int64)
    assert np.abs(sums).max(initial=0) < 2**40
    hi, lo = sums[:len(w)].astype(object), sums[len(w):].astype(object)
    return np.array((hi * (1 << 32) + lo) % q, dtype=np.uint64).reshape(len(w), -1)


def conjugation(n, cyclic):
    """g = N - 1."""
    return galois.galois_order(n, 1 if cyclic else -1) - 1


def back_project(oracle, q, n, width, weights, count, keys, components, domain=17, index_base=0, conjugate=False, cyclic=False):
    """weights [groups][sets][256] -> (uint64 [count, sets, width, n], int32 [count]).  Vector j uses keys[j // components],
    weights[j // components] and the streams index_base + 256 (j % components) + r, exactly as ring_norm_model.project."""
    groups = -(-count // components)
    assert components >= 1 and len(keys) >= groups and len(weights) >= groups
    sets, length = len(weights[0]), width * n
    assert 1 <= sets <= MAX_SETS and length <= 2**32
    out, status = np.zeros((count, sets, width, n), dtype=np.uint64), np.ones(count, dtype=np.int32)
    for j in range(count):
        group = j // components
        if any(int(v) >= q for row in weights[group] for v in row):
            status[j] = -1
            continue
        signs = signs_of(oracle, length, keys[group], domain, index_base + ROWS * (j % components))
        out[j] = weighted_columns(signs, weights[group], q).reshape(sets, width, n)
        if conjugate:
            out[j] = galois.automorphism_np(out[j], conjugation(n, cyclic), q, 1 if cyclic else -1)
    return out, status


def back_project_ints(oracle, q, length, weights, key, domain=17, index=0):
    """One set of one vector, term by term in Python integers: [length] ints."""
    streams = [Stream(oracle, key, domain, index + r) for r in range(ROWS)]
    return [sum(int(weights[r]) * norm.entry(streams[r].word(pos // 32), pos % 32) for r in range(ROWS)) % q for pos in range(length)]


# ---- the model's own tests (collected by tests/test_ring_backproject_abi.py) ------------------------------------------------------------
def test_weighted_columns_by_hand_on_one_stream_word():
    q = 97
    word0 = 0b11_10_01_00                                          # fields 0 .. 3 = 0, 1, 2, 3 -> 0, +1, -1, 0
    word1 = 0b10_10_01_01                                          # 1, 1, 2, 2 -> +1, +1, -1, -1

    class OneWord:
        def __init__(self, word):
            self.word = word

        def words(self, first, count):
            assert (first, count) == (0, 1)
            return np.array([self.word], dtype=np.uint64)
    signs = np.zeros((ROWS, 4), dtype=np.int8)
    signs[0], signs[1] = norm.row_signs(OneWord(word0), 4), norm.row_signs(OneWord(word1), 4)
    assert signs[0].tolist() == [0, 1, -1, 0] and signs[1].tolist() == [1, 1, -1, -1]
    w = [0] * ROWS
    w[0], w[1] = 5, q - 2                                          # 5 pi_0 - 2 pi_1 = [-2, 3, -3, 2]
    assert weighted_columns(signs, [w], q).tolist() == [[q - 2, 3, q - 3, 2]]
    # the conjugation of that one element of X^4 + 1, by hand: x_0, -x_3, -x_2, -x_1; of X^4 - 1: x_0, x_3, x_2, x_1
    x = np.array([q - 2, 3, q - 3, 2], dtype=np.uint64)
    assert conjugation(4, False) == 7 and conjugation(4, True) == 3
    assert galois.automorphism_np(x, 7, q, -1).tolist() == [q - 2, q - 2, 3, q - 3]
    assert galois.automorphism_np(x, 3, q, 1).tolist() == [q - 2, 2, q - 3, 3]
    assert galois.automorphism_np(x, 7, q, -1).tolist() == galois.automorphism(x.tolist(), 7, q, -1)


def test_unit_weight_gives_the_matrix_row(oracle):
    q, n, width = 12289, 8, 5                                      # len 40: crosses a word and ends inside one
    keys = [key_from_seed(3), key_from_bytes(bytes(range(32)))]
    for r in (0, 31, 255):
        e = [[[1 if i == r else 0 for i in range(ROWS)]]] * 2
        out, status = back_project(oracle, q, n, width, e, 3, keys, 2, 17, 9)
        assert status.tolist() == [1, 1, 1]
        for j in range(3):
            row = norm.project_matrix(oracle, q, n, width, keys[j // 2], r, 1, 17, 9 + ROWS * (j % 2))
            assert np.array_equal(out[j, 0], row[0]), (r, j)


def test_adjoint_identity_against_the_projection(oracle):
    """sum_pos out[pos] centred(s[pos]) = sum_r w_r p_r (mod q): <Pi^T w, s> = <w, Pi s>."""
    for q, n, width, cyclic in [(12289, 8, 5, False), (17592169062401, 64, 5, False), (GOLD, 16, 3, True)]:
        rng = np.random.default_rng(n)
        count, components, bound = 3, 2, 1000
        keys = [key_from_seed(n), key_from_seed(n + 1)]
        s = np.array(rng.integers(-bound, bound + 1, size=(count, width, n)).astype(object) % q, dtype=np.uint64)
        p, p_status = norm.project(oracle, q, s, bound, keys, components, 17, 5)
        assert p_status.tolist() == [1] * count
        weights = [[[int(v) for v in rng.integers(0, min(q, 2**63), size=ROWS)] for _ in range(2)] for _ in range(2)]
        out, status = back_project(oracle, q, n, width, weights, count, keys, components, 17, 5)
        assert status.tolist() == [1] * count
        for j in range(count):
            c = [norm.centred(v, q) for v in s[j].reshape(-1).tolist()]
            for k in range(2):
                lhs = sum(o * v for o, v in zip(out[j, k].reshape(-1).tolist(), c)) % q
                assert lhs == sum(w * int(v) for w, v in zip(weights[j // components][k], p[j].tolist())) % q, (q, j, k)
        # the conjugated form is the automorphism of the plain one, element by element (the list model: the definition)
        conj, _ = back_project(oracle, q, n, width, weights, count, keys, components, 17, 5, True, cyclic)
        sign = 1 if cyclic else -1
        assert conj[2, 1].tolist() == [galois.automorphism(e, conjugation(n, cyclic), q, sign) for e in out[2, 1].tolist()]


def test_all_weights_q_minus_1_at_the_widest_moduli(oracle):
    """Every weight q - 1: the sums reach 256 (q - 1), past 64 bits — against the sum in Python integers."""
    for q in (Q60, GOLD):
        key, length = key_from_seed(60), 40
        w = [q - 1] * ROWS
        want = back_project_ints(oracle, q, length, w, key, 17, 3)
        out, status = back_project(oracle, q, 8, 5, [[w]], 1, [key], 1, 17, 3)
        assert status.tolist() == [1] and out.reshape(-1).tolist() == want
        signs = signs_of(oracle, length, key, 17, 3).astype(object)
        assert want == [(-int(c)) % q for c in signs.sum(axis=0)] and len(set(want)) > 3      # (q - 1) = -1: minus the column sums


def test_status_rule(oracle):
    q = 12289
    ok, bad = [[1] * ROWS, [q - 1] * ROWS], [[1] * ROWS, [0] * 255 + [q]]
    out, status = back_project(oracle, q, 8, 1, [ok, bad, ok], 5, [key_from_seed(i) for i in range(3)], 2)
    assert status.tolist() == [1, 1, -1, -1, 1] and not out[2:4].any() and out[0].any() and out[4].any()
