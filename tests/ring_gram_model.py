"""References for the ring Gram matrices (lsr_ntt_ring_gram_batch), pure CPU and pure Python:
g[j][i][l] = sum_{c < width} a[j][i][c] * b[j][l][c] in Z_q[X]/(X^n + 1) (sign = -1) or Z_q[X]/(X^n - 1) (sign = +1).

  * packed_index:     the polynomial of the pair (i, l), i <= l, in the packed upper triangle of the symmetric form;
  * schoolbook_gram:  the definition on Python integers, cross form ([batch][ra][rb][n]) or, b=None, packed ([batch][r (r + 1) / 2][n]);
  * dot_pairs:        the gathered operands of the route the call replaces, [batch * pairs][width][n] each, pairs in output order;
  * oracle_gram:      a second reference that shares nothing with the schoolbook — the CPU oracle's transforms (every operand polynomial
                      once) around pointwise sums, ring_tile_model's _transform / _pointwise_sum: Goldilocks and the cyclic rings go
                      through Python integers, the negacyclic ones through the oracle's mul_pointwise.
The tests at the bottom (no GPU) pin the index against enumeration, the packed form against the cross form and one case by hand, and
hold the two references against each other in every flavour of ring_tile_model.FLAVOURS before either judges a kernel."""
import numpy as np
import pytest

from ring_tile_model import FLAVOURS, GOLDILOCKS, _pointwise_sum, _transform, goldilocks_lazy_carry, omega_for, planted


def packed_index(r, i, l):
    assert 0 <= i <= l < r
    return i * r - i * (i - 1) // 2 + (l - i)


def _mul(x, y, q, sign):
    n = len(x)
    full = [0] * (2 * n)                       # the plain product, degree < 2 n - 1; X^(n + k) folds onto sign * X^k
    for s, xs in enumerate(x):
        if xs:
            full[s:s + n] = [f + xs * yt for f, yt in zip(full[s:s + n], y)]
    return [(lo + sign * hi) % q for lo, hi in zip(full[:n], full[n:])]


def _dot(u, v, q, sign):
    """sum_c u[c] * v[c] for two vectors [width][n] of Python integers"""
    n = len(u[0])
    acc = [0] * n
    for x, y in zip(u, v):
        acc = [(s + t) % q for s, t in zip(acc, _mul(x, y, q, sign))]
    return acc


def pairs(ra, rb, symmetric):
    """(i, l) in the order the outputs of one family are stored"""
    return [(i, l) for i in range(ra) for l in range(i if symmetric else 0, rb)]


def schoolbook_gram(a, b, q, sign):
    """a: [batch][ra][width][n], b: [batch][rb][width][n] or None -> nested lists [batch][ra][rb][n], or [batch][r (r + 1) / 2][n]"""
    a = np.asarray(a, dtype=np.uint64).tolist()
    if b is None:
        r = len(a[0])
        return [[_dot(fam[i], fam[l], q, sign) for i, l in pairs(r, r, True)] for fam in a]
    b = np.asarray(b, dtype=np.uint64).tolist()
    return [[[_dot(u, v, q, sign) for v in fb] for u in fa] for fa, fb in zip(a, b)]


def dot_pairs(a, b):
    """The operands of lsr_ntt_ring_dot_batch for every output of the Gram call, in output order: (a', b'), each
    [batch * pairs][width][n]."""
    a = np.asarray(a, dtype=np.uint64)
    symmetric = b is None
    b = a if symmetric else np.asarray(b, dtype=np.uint64)
    batch, ra, width, n = a.shape
    idx = pairs(ra, b.shape[1], symmetric)
    ii, ll = [i for i, _ in idx], [l for _, l in idx]
    return (np.ascontiguousarray(a[:, ii]).reshape(batch * len(idx), width, n),
            np.ascontiguousarray(b[:, ll]).reshape(batch * len(idx), width, n))


# ---- the oracle's transforms around pointwise sums ------------------------------------------------------------------------------------
def oracle_pair_sums(oracle, q, n, fa, fb, idx, cyclic):
    """fa [batch, ra, terms, n], fb [batch, rb, terms, n] in the evaluation domain, idx a list of (i, l) -> [batch, len(idx), n]:
    sum_c fa[j][i][c] . fb[j][l][c] per pair, canonical."""
    ii, ll = [i for i, _ in idx], [l for _, l in idx]
    return _pointwise_sum(oracle, q, n, np.ascontiguousarray(fa[:, ii]), np.ascontiguousarray(fb[:, ll]), cyclic)


def oracle_gram(oracle, q, n, a, b, cyclic, omega):
    """a: [batch, ra, width, n], b: [batch, rb, width, n] or None -> uint64 [batch, ra, rb, n], or packed [batch, r (r + 1) / 2, n]:
    INTT(sum_c NTT(a_i[c]) . NTT(b_l[c])), every operand polynomial transformed once."""
    fa = _transform(oracle, q, n, a, cyclic, omega)
    symmetric = b is None
    fb = fa if symmetric else _transform(oracle, q, n, b, cyclic, omega)
    batch, ra, rb = fa.shape[0], fa.shape[1], fb.shape[1]
    sums = oracle_pair_sums(oracle, q, n, fa, fb, pairs(ra, rb, symmetric), cyclic)
    out = _transform(oracle, q, n, sums, cyclic, omega, inverse=True)
    return out if symmetric else out.reshape(batch, ra, rb, n)


# ---- the model's own tests (CPU only; collected through tests/test_ring_gram_abi.py) ----------------------------------------------------
@pytest.mark.parametrize("n", [2, 16])
@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_oracle_gram_equals_schoolbook(oracle, flavour, n):
    (q, cyclic), omega = FLAVOURS[flavour], omega_for(oracle, flavour, n)
    sign = 1 if cyclic else -1
    rng = np.random.default_rng(n + len(flavour))
    batch, r, rb, width = 2, 5, 3, 2
    a = planted(rng, q, batch * r * width, n).reshape(batch, r, width, n)
    b = planted(rng, q, batch * rb * width, n).reshape(batch, rb, width, n)
    if q == GOLDILOCKS and n >= 4:
        a[0, 1, 0] = b[1, 2, 0] = goldilocks_lazy_carry(n)
    assert oracle_gram(oracle, q, n, a, b, cyclic, omega).tolist() == schoolbook_gram(a, b, q, sign), (flavour, n, "cross")
    assert oracle_gram(oracle, q, n, a, None, cyclic, omega).tolist() == schoolbook_gram(a, None, q, sign), (flavour, n, "symmetric")
    assert oracle_gram(oracle, q, n, a, a, cyclic, omega).tolist() == schoolbook_gram(a, a, q, sign), (flavour, n, "b is a")


def test_packed_index_matches_enumeration():
    for r in range(1, 7):
        order = pairs(r, r, True)
        assert len(order) == r * (r + 1) // 2
        assert [packed_index(r, i, l) for i, l in order] == list(range(len(order))), r


def test_symmetric_form_is_the_upper_triangle_of_the_cross_form():
    rng = np.random.default_rng(5)
    for q, n, sign in [(97, 4, -1), (12289, 8, -1), (97, 4, 1)]:
        a = rng.integers(0, q, size=(2, 3, 2, n), dtype=np.uint64)
        full = schoolbook_gram(a, a, q, sign)
        packed = schoolbook_gram(a, None, q, sign)
        for j in range(2):
            for i in range(3):
                for l in range(3):
                    assert full[j][i][l] == full[j][l][i]
                    if i <= l:
                        assert packed[j][packed_index(3, i, l)] == full[j][i][l], (q, n, j, i, l)
    u, v = dot_pairs(a, None)
    assert u.shape == v.shape == (2 * 6, 2, n)
    assert u[6 + packed_index(3, 1, 2)].tolist() == a[1, 1].tolist() and v[6 + packed_index(3, 1, 2)].tolist() == a[1, 2].tolist()


def test_gram_by_hand():
    """n = 2, q = 97, width 2, two vectors s_0 = (1 + 2X, 3), s_1 = (X, 4 + 5X).  Mod X^2 + 1:
    <s_0, s_0> = (1 + 2X)^2 + 9 = 1 + 4X - 4 + 9 = 6 + 4X;  <s_0, s_1> = (1 + 2X) X + 3 (4 + 5X) = X - 2 + 12 + 15X = 10 + 16X;
    <s_1, s_1> = X^2 + (4 + 5X)^2 = -1 + 16 + 40X - 25 = -10 + 40X.  Mod X^2 - 1 every X^2 is +1."""
    a = np.array([[[[1, 2], [3, 0]], [[0, 1], [4, 5]]]], dtype=np.uint64)
    assert schoolbook_gram(a, None, 97, -1) == [[[6, 4], [10, 16], [87, 40]]]
    assert schoolbook_gram(a, a, 97, -1) == [[[[6, 4], [10, 16]], [[10, 16], [87, 40]]]]
    assert schoolbook_gram(a, None, 97, 1) == [[[14, 4], [14, 16], [42, 40]]]
