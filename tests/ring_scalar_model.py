"""Python-integer model of the scalar-weighted aggregation of ring vectors (lsr_ntt_ring_scalar_combine_batch, batch.h
"scalar-weighted aggregation of ring vectors").  TEST INFRASTRUCTURE.  It reads nothing from the library.

    out[j][k][pos] = (addend ? addend[j][k][pos] : 0) + sum_i weights[j // components][k][i] v[j term_stride + i][pos]  mod q

Exactness: the words travel as numpy OBJECT arrays of Python integers, so a product of two 64-bit words and a sum of 65536 of them are
exact; numpy only vectorises the loop over the positions ([sets, terms] @ [terms, len] on object arrays runs Python's * and +)."""
import numpy as np

MAX_SETS = 16
Q14 = 12289
Q44 = 17592169062401
Q60 = 1152921504606584833
GOLD = 2**64 - 2**32 + 1


def _objects(x):
    return np.array(np.asarray(x, dtype=np.uint64).tolist(), dtype=object).reshape(np.shape(x))


def scalar_combine(q, n, width, v, weights, addend, count, term_stride, components):
    """v [vectors, width, n], weights [groups, sets, terms], addend None or [count, sets, width, n] (words below 2^64) ->
    (uint64 [count, sets, width, n], int32 [count]).  Vector j uses weights[j // components] and v[j term_stride + i], i < terms."""
    w = np.asarray(weights, dtype=np.uint64)
    groups, sets, terms = w.shape
    length = width * n
    assert components >= 1 and groups >= -(-count // components) and 1 <= sets <= MAX_SETS and terms >= 1
    vo = _objects(np.asarray(v, dtype=np.uint64).reshape(-1, length))
    assert vo.shape[0] >= (count - 1) * term_stride + terms
    wo = _objects(w)
    ao = None if addend is None else _objects(np.asarray(addend, dtype=np.uint64).reshape(count, sets, length))
    out, status = np.zeros((count, sets, width, n), dtype=np.uint64), np.ones(count, dtype=np.int32)
    for j in range(count):
        group = j // components
        if any(x >= q for x in wo[group].reshape(-1)):
            status[j] = -1
            continue
        total = wo[group] @ vo[j * term_stride:j * term_stride + terms]
        if ao is not None:
            total = total + ao[j]
        out[j] = np.array((total % q).tolist(), dtype=np.uint64).reshape(sets, width, n)
    return out, status


# ---- the model's own tests (collected by tests/test_ring_scalar_abi.py) -----------------------------------------------------------------
def test_two_by_two_by_hand():
    q = 97
    v = [[[1, 2]], [[3, 96]]]                                      # two vectors of one element of n = 2
    weights = [[[5, 7], [96, 1]]]                                  # set 0: 5 v0 + 7 v1; set 1: -v0 + v1
    out, status = scalar_combine(q, 2, 1, v, weights, None, 1, 0, 1)
    assert status.tolist() == [1]
    assert out.tolist() == [[[[(5 + 21) % q, (10 + 7 * 96) % q]], [[2, (96 - 2) % q]]]]
    assert out.tolist() == [[[[26, 3]], [[2, 94]]]]
    addend = [[[[96, 1]], [[95, 3]]]]
    out, _ = scalar_combine(q, 2, 1, v, weights, addend, 1, 0, 1)
    assert out.tolist() == [[[[25, 4]], [[0, 0]]]]
    # two outputs with term_stride 1 over three vectors: output 1 takes v1, v2
    v3 = v + [[[10, 20]]]
    out, _ = scalar_combine(q, 2, 1, v3, weights, None, 2, 1, 2)
    assert out[0].tolist() == [[[26, 3]], [[2, 94]]]
    assert out[1].tolist() == [[[(15 + 70) % q, (5 * 96 + 140) % q]], [[7, (20 - 96) % q]]]


def test_status_rule():
    q = Q14
    rng = np.random.default_rng(1)
    v = rng.integers(0, q, size=(3, 1, 8), dtype=np.uint64)
    ok, bad = [[1, 2, 3], [q - 1, 0, 5]], [[1, 2, 3], [4, q, 5]]
    out, status = scalar_combine(q, 8, 1, v, [ok, bad, ok], None, 5, 0, 2)
    assert status.tolist() == [1, 1, -1, -1, 1] and not out[2:4].any() and out[0].any() and out[4].any()
    addend = np.full((5, 2, 1, 8), 7, dtype=np.uint64)
    out, status = scalar_combine(q, 8, 1, v, [ok, bad, ok], addend, 5, 0, 2)
    assert status.tolist() == [1, 1, -1, -1, 1] and not out[2:4].any()            # zeros, not the addend


def test_unit_weight_returns_the_term_plus_the_addend():
    for q in (Q14, Q44, Q60, GOLD):
        rng = np.random.default_rng(q % 1000)
        v = rng.integers(0, q, size=(7, 2, 4), dtype=np.uint64)
        addend = rng.integers(0, q, size=(2, 3, 2, 4), dtype=np.uint64)
        weights = np.zeros((1, 3, 3), dtype=np.uint64)
        weights[0, 0, 0] = weights[0, 1, 1] = weights[0, 2, 2] = 1
        out, status = scalar_combine(q, 4, 2, v, weights, None, 2, 4, 2)
        assert status.tolist() == [1, 1]
        for j in range(2):
            for k in range(3):
                assert np.array_equal(out[j, k], v[4 * j + k]), (q, j, k)
        out, _ = scalar_combine(q, 4, 2, v, weights, addend, 2, 4, 2)
        for j in range(2):
            for k in range(3):
                want = (v[4 * j + k].astype(object) + addend[j, k].astype(object)) % q
                assert out[j, k].tolist() == want.tolist(), (q, j, k)


def test_all_words_q_minus_1():
    """(q - 1)^2 = 1: terms of them sum to terms mod q, and an addend of q - 1 takes one off."""
    for q in (Q14, Q44, Q60, GOLD):
        for terms in (1, 33, 65):
            v = np.full((terms, 1, 2), q - 1, dtype=np.uint64)
            weights = np.full((1, 2, terms), q - 1, dtype=np.uint64)
            out, status = scalar_combine(q, 2, 1, v, weights, None, 1, 0, 1)
            assert status.tolist() == [1] and set(out.reshape(-1).tolist()) == {terms % q}
            addend = np.full((1, 2, 1, 2), q - 1, dtype=np.uint64)
            out, _ = scalar_combine(q, 2, 1, v, weights, addend, 1, 0, 1)
            assert set(out.reshape(-1).tolist()) == {(terms - 1) % q}
