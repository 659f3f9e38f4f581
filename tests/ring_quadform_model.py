"""References for the ring quadratic forms and the symmetrised packed Gram matrix (lsr_ntt_ring_quadform_batch,
lsr_ntt_ring_gram_sym2_batch), pure CPU and pure Python, on top of ring_gram_model:

  * schoolbook_quadform:  out[j] = sum_i g[j][(i,i)] c_i c_i + offdiag * sum_{i<l} g[j][(i,l)] c_i c_l on Python integers;
  * schoolbook_sym2:      h[j][(i,l)] = <a_i, b_l> + <a_l, b_i> (i < l), h[j][(i,i)] = <a_i, b_i>, packed;
  * composed_operands:    the operands of the route the quadratic form replaces — the factors of the pair products c_i * c_l in
                          packed order and the scalar each product is scaled by (1 on the diagonal, offdiag off it);
  * composed_quadform, composed_sym2:  the composed routes run on a context's own ring_mul / ring_dot;
  * oracle_sym2, oracle_quadform:      second references that share nothing with the schoolbook — the CPU oracle's transforms (every
                          operand polynomial once) around pointwise sums, as ring_gram_model.oracle_gram;
  * flat_gram, flat_sym2, flat_quadform:  the closed forms of the flat-spectrum cases, whose operands are constant polynomials.
The tests at the bottom (no GPU) pin one case by hand, sym2 against the cross form and the quadratic form of a Gram matrix against
<z, z> of the folded vector, hold the oracle references against the schoolbook in every flavour of ring_tile_model.FLAVOURS, and the
closed forms against the schoolbook."""
import numpy as np
import pytest

from ring_gram_model import _dot, _mul, dot_pairs, oracle_pair_sums, packed_index, pairs, schoolbook_gram
from ring_tile_model import FLAVOURS, GOLDILOCKS, _pointwise_sum, _transform, goldilocks_lazy_carry, omega_for, planted


def _add(x, y, q):
    return [(s + t) % q for s, t in zip(x, y)]


def schoolbook_quadform_parts(g, c, q, sign):
    """(diag, off), each nested lists [batch][n]: diag[j] = sum_i g[j][(i,i)] c_i c_i and off[j] = sum_{i<l} g[j][(i,l)] c_i c_l.
    g: [batch][r (r + 1) / 2][n], c: [batch][r][n] or [r][n] (shared)."""
    g = np.asarray(g, dtype=np.uint64).tolist()
    c = np.asarray(c, dtype=np.uint64).tolist()
    if not isinstance(c[0][0], list):
        c = [c] * len(g)
    diag, off = [], []
    for fam, cs in zip(g, c):
        r, n = len(cs), len(cs[0])
        acc = {True: [0] * n, False: [0] * n}
        for i, l in pairs(r, r, True):
            acc[i == l] = _add(acc[i == l], _mul(fam[packed_index(r, i, l)], _mul(cs[i], cs[l], q, sign), q, sign), q)
        diag.append(acc[True])
        off.append(acc[False])
    return diag, off


def schoolbook_quadform(g, c, q, sign, offdiag):
    """out[j] = diag[j] + offdiag * off[j] mod q -> nested lists [batch][n]"""
    diag, off = schoolbook_quadform_parts(g, c, q, sign)
    return [[(d + offdiag * o) % q for d, o in zip(dj, oj)] for dj, oj in zip(diag, off)]


def schoolbook_sym2(a, b, q, sign):
    """a, b: [batch][r][width][n] -> nested lists [batch][r (r + 1) / 2][n]"""
    a, b = np.asarray(a, dtype=np.uint64).tolist(), np.asarray(b, dtype=np.uint64).tolist()
    r = len(a[0])
    return [[_dot(fa[i], fb[i], q, sign) if i == l else _add(_dot(fa[i], fb[l], q, sign), _dot(fa[l], fb[i], q, sign), q)
             for i, l in pairs(r, r, True)] for fa, fb in zip(a, b)]


def composed_operands(c, batch, offdiag):
    """c: [c_rows][r][n] with c_rows 1 or batch -> (left, right, scale): left and right [batch * pairs][n], the factors of the products
    c_i * c_l in packed order family by family; scale [pairs], the word each product is multiplied by before the inner product with g."""
    c = np.asarray(c, dtype=np.uint64)
    c = np.broadcast_to(c, (batch,) + c.shape[1:])
    r, n = c.shape[1], c.shape[2]
    idx = pairs(r, r, True)
    ii, ll = [i for i, _ in idx], [l for _, l in idx]
    scale = [1 if i == l else offdiag for i, l in idx]
    return np.ascontiguousarray(c[:, ii]).reshape(batch * len(idx), n), np.ascontiguousarray(c[:, ll]).reshape(batch * len(idx), n), scale


def _to_u64(values):
    return np.array(values.tolist(), dtype=np.uint64).reshape(values.shape)


def composed_quadform(ctx, q, g, c, offdiag):
    """The route the quadratic form replaces, on a context's own calls: ring_mul per pair, the scaling by offdiag mod q (numpy),
    ring_dot with terms = pairs.  g [batch][pairs][n], c [c_rows][r][n] -> [batch][n]."""
    batch, npairs, n = g.shape
    left, right, scale = composed_operands(c, batch, offdiag)
    prod = ctx.ring_mul(left, right).reshape(batch, npairs, n)
    if max(scale) * q < 1 << 64:
        scaled = prod * np.array(scale, dtype=np.uint64)[None, :, None] % np.uint64(q)
    else:
        scaled = _to_u64(prod.astype(object) * np.array(scale, dtype=object)[None, :, None] % q)
    return ctx.ring_dot(g, np.ascontiguousarray(scaled))


def composed_sym2(ctx, q, a, b):
    """ring_dot per ordered pair (i, l), then x_il + x_li mod q off the diagonal and x_ii on it, packed (q < 2^63).
    a, b [batch][r][width][n] -> [batch][r (r + 1) / 2][n]."""
    batch, r, _, n = a.shape
    u, v = dot_pairs(a, b)
    x = ctx.ring_dot(u, v).reshape(batch, r, r, n)
    return np.stack([x[:, i, i] if i == l else (x[:, i, l] + x[:, l, i]) % np.uint64(q) for i, l in pairs(r, r, True)], axis=1)


# ---- the oracle's transforms around pointwise sums ------------------------------------------------------------------------------------
def _add_words(x, y, q):
    """x + y mod q for canonical uint64 arrays (Goldilocks sums pass 2^64: Python integers)"""
    if q < 1 << 63:
        s = x + y
        return s - np.uint64(q) * (s >= np.uint64(q)).astype(np.uint64)
    return np.array([(int(u) + int(v)) % q for u, v in zip(x.ravel(), y.ravel())], dtype=np.uint64).reshape(x.shape)


def oracle_sym2(oracle, q, n, a, b, cyclic, omega):
    """a, b: [batch, r, width, n] -> uint64 [batch, r (r + 1) / 2, n]: INTT(sum_c NTT(a_i[c]) . NTT(b_l[c]) + NTT(a_l[c]) . NTT(b_i[c])) off
    the diagonal, INTT(sum_c NTT(a_i[c]) . NTT(b_i[c])) on it; every operand polynomial transformed once."""
    fa = _transform(oracle, q, n, a, cyclic, omega)
    fb = fa if b is a else _transform(oracle, q, n, b, cyclic, omega)
    idx = pairs(fa.shape[1], fa.shape[1], True)
    sums = oracle_pair_sums(oracle, q, n, fa, fb, idx, cyclic)
    off = [k for k, (i, l) in enumerate(idx) if i != l]
    if off:
        sums[:, off] = _add_words(sums[:, off], oracle_pair_sums(oracle, q, n, fa, fb, [(idx[k][1], idx[k][0]) for k in off], cyclic), q)
    return _transform(oracle, q, n, sums, cyclic, omega, inverse=True)


def oracle_quadform_parts(oracle, q, n, g, c, cyclic, omega):
    """(diag, off), each uint64 [batch, n], as schoolbook_quadform_parts: the pair products NTT(c_i) . NTT(c_l) pointwise, their sums
    against NTT(g) over the diagonal and over the rest of the triangle, one inverse transform each."""
    fg = _transform(oracle, q, n, g, cyclic, omega)
    fc = _transform(oracle, q, n, c, cyclic, omega)
    batch, r = fg.shape[0], fc.shape[-2]
    fc = np.broadcast_to(fc, (batch, r, n))
    idx = pairs(r, r, True)
    ii, ll = [i for i, _ in idx], [l for _, l in idx]
    cc = _pointwise_sum(oracle, q, n, np.ascontiguousarray(fc[:, ii, None]), np.ascontiguousarray(fc[:, ll, None]), cyclic)
    parts = []
    for want_diag in (True, False):
        sel = [k for k, (i, l) in enumerate(idx) if (i == l) == want_diag]
        if not sel:
            parts.append(np.zeros((batch, n), dtype=np.uint64))
            continue
        sums = _pointwise_sum(oracle, q, n, np.ascontiguousarray(fg[:, sel]), np.ascontiguousarray(cc[:, sel]), cyclic)
        parts.append(_transform(oracle, q, n, sums, cyclic, omega, inverse=True))
    return parts[0], parts[1]


def combine_parts(parts, q, offdiag):
    """diag + offdiag * off mod q on Python integers -> uint64 [batch, n]"""
    diag, off = parts
    words = [(int(d) + offdiag * int(o)) % q for d, o in zip(np.ravel(diag), np.ravel(off))]
    return np.array(words, dtype=np.uint64).reshape(np.shape(diag))


def oracle_quadform(oracle, q, n, g, c, offdiag, cyclic, omega):
    """g: [batch, r (r + 1) / 2, n], c: [batch, r, n] or [r, n] (shared) -> uint64 [batch, n]"""
    return combine_parts(oracle_quadform_parts(oracle, q, n, g, c, cyclic, omega), q, offdiag)


# ---- the flat-spectrum cases: constant polynomials --------------------------------------------------------------------------------------
def constant(shape, n, u):
    """uint64 [*shape, n]: every polynomial the constant u.  Its transform is u at every position, in every one of these rings."""
    x = np.zeros(tuple(shape) + (n,), dtype=np.uint64)
    x[..., 0] = u
    return x


def flat_pairs(q):
    """(u, v) with u v mod q = floor(q/2), floor(q/2) + 1, q - 1, 1: the first two are centred +q/2 resp. -q/2 (q odd)"""
    pairs_ = [((q + 1) // 2, q - 1), ((q + 1) // 2, 1), (q - 1, 1), (1, 1)]
    assert [u * v % q for u, v in pairs_] == [q // 2, q // 2 + 1, q - 1, 1]
    return pairs_


def flat_gram(q, width, u, v):
    """coefficient 0 of every Gram output of all-u against all-v vectors (the other coefficients are 0)"""
    return width * u * v % q


def flat_sym2(q, width, u, v, diagonal):
    return (1 if diagonal else 2) * width * u * v % q


def flat_quadform(q, r, offdiag, gamma, kappa):
    """coefficient 0 of the quadratic form with every g the constant gamma and every c the constant kappa"""
    return (r + offdiag * (r * (r - 1) // 2)) * gamma * kappa * kappa % q


# ---- the model's own tests (CPU only; collected through tests/test_ring_quadform_abi.py) -----------------------------------------------
@pytest.mark.parametrize("n", [2, 16])
@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_oracle_references_equal_schoolbook(oracle, flavour, n):
    (q, cyclic), omega = FLAVOURS[flavour], omega_for(oracle, flavour, n)
    sign = 1 if cyclic else -1
    rng = np.random.default_rng(n + len(flavour) + 1)
    batch, r, width = 2, 5, 2
    npairs = r * (r + 1) // 2
    a = planted(rng, q, batch * r * width, n).reshape(batch, r, width, n)
    b = planted(rng, q, batch * r * width, n).reshape(batch, r, width, n)
    g = planted(rng, q, batch * npairs, n).reshape(batch, npairs, n)
    c = planted(rng, q, batch * r, n).reshape(batch, r, n)
    if q == GOLDILOCKS and n >= 4:
        a[0, 1, 0] = b[1, 2, 0] = g[0, 3] = c[1, 1] = goldilocks_lazy_carry(n)
    assert oracle_sym2(oracle, q, n, a, b, cyclic, omega).tolist() == schoolbook_sym2(a, b, q, sign), (flavour, n, "sym2")
    assert oracle_sym2(oracle, q, n, a, a, cyclic, omega).tolist() == schoolbook_sym2(a, a, q, sign), (flavour, n, "sym2, b is a")
    for cc in (c, c[1]):
        for offdiag in (1, 2, (q + 1) // 2, q - 1):
            got = oracle_quadform(oracle, q, n, g, cc, offdiag, cyclic, omega)
            assert got.tolist() == schoolbook_quadform(g, cc, q, sign, offdiag), (flavour, n, cc.ndim, offdiag)
    assert oracle_quadform(oracle, q, n, g[:, :1], c[:, :1], 2, cyclic, omega).tolist() == schoolbook_quadform(g[:, :1], c[:, :1], q, sign, 2)


def test_flat_spectrum_closed_forms_equal_schoolbook():
    n, r, width = 4, 3, 5
    for q, _ in set(FLAVOURS.values()):
        for sign in (-1, 1):
            for u, v in flat_pairs(q):
                a, b = constant((1, r, width), n, u), constant((1, r, width), n, v)
                rest = [0] * (n - 1)
                assert schoolbook_gram(a, b, q, sign) == [[[[flat_gram(q, width, u, v)] + rest] * r] * r]
                assert schoolbook_sym2(a, b, q, sign) == [[[flat_sym2(q, width, u, v, i == l)] + rest for i, l in pairs(r, r, True)]]
                g, c = constant((1, r * (r + 1) // 2), n, u), constant((1, r), n, v)
                for offdiag in (1, 2, q - 1):
                    assert schoolbook_quadform(g, c, q, sign, offdiag) == [[flat_quadform(q, r, offdiag, u, v)] + rest], (q, sign, u, v, offdiag)


def test_quadform_by_hand():
    """n = 2, q = 97, r = 2, c_0 = 1 + X, c_1 = 2, g = (g_00, g_01, g_11) = (3, X, 1 + 2X), offdiag = 2.
    Mod X^2 + 1: c_0^2 = 2X, c_0 c_1 = 2 + 2X, c_1^2 = 4;  3 * 2X = 6X;  2 * X (2 + 2X) = 4X - 4;  (1 + 2X) * 4 = 4 + 8X;  sum 18X.
    Mod X^2 - 1: c_0^2 = 2 + 2X;  3 (2 + 2X) = 6 + 6X;  2 * X (2 + 2X) = 4X + 4;  4 + 8X;  sum 14 + 18X.
    offdiag = 1 takes the middle term once: 2 + 16X (mod X^2 + 1: X (2 + 2X) = 2X - 2)."""
    g = np.array([[[3, 0], [0, 1], [1, 2]]], dtype=np.uint64)
    c = np.array([[1, 1], [2, 0]], dtype=np.uint64)
    assert schoolbook_quadform(g, c, 97, -1, 2) == [[0, 18]]
    assert schoolbook_quadform(g, c, 97, 1, 2) == [[14, 18]]
    assert schoolbook_quadform(g, c[None], 97, -1, 1) == [[2, 16]]
    left, right, scale = composed_operands(c[None], 1, 2)
    assert left.tolist() == [[1, 1], [1, 1], [2, 0]] and right.tolist() == [[1, 1], [2, 0], [2, 0]] and scale == [1, 2, 1]


def test_sym2_is_the_cross_form_plus_its_transpose():
    rng = np.random.default_rng(7)
    for q, n, sign in [(97, 4, -1), (12289, 8, -1), (97, 4, 1)]:
        a = rng.integers(0, q, size=(2, 3, 2, n), dtype=np.uint64)
        b = rng.integers(0, q, size=(2, 3, 2, n), dtype=np.uint64)
        x = schoolbook_gram(a, b, q, sign)
        h = schoolbook_sym2(a, b, q, sign)
        for j in range(2):
            for i, l in pairs(3, 3, True):
                want = x[j][i][i] if i == l else _add(x[j][i][l], x[j][l][i], q)
                assert h[j][packed_index(3, i, l)] == want, (q, n, j, i, l)


def test_quadform_of_a_gram_matrix_is_the_norm_of_the_fold():
    """z = sum_i c_i s_i:  <z, z> = sum_{i,l} <s_i, s_l> c_i c_l, the packed triangle with offdiag = 2; and with h = sym2(phi, s),
    offdiag = 1:  sum_i <phi_i, z> c_i = <sum_i c_i phi_i, z>."""
    rng = np.random.default_rng(11)
    for q, n, sign in [(97, 4, -1), (12289, 8, -1), (97, 4, 1)]:
        r, width = 3, 2
        s = rng.integers(0, q, size=(1, r, width, n), dtype=np.uint64)
        phi = rng.integers(0, q, size=(1, r, width, n), dtype=np.uint64)
        c = rng.integers(0, q, size=(r, n), dtype=np.uint64)
        fold = lambda v: [[sum(np.array(_mul(c[i].tolist(), v[0, i, k].tolist(), q, sign), dtype=object) for i in range(r)) % q  # noqa: E731
                           for k in range(width)]]
        z, f = [[list(map(int, p)) for p in fold(s)[0]]], [[list(map(int, p)) for p in fold(phi)[0]]]
        assert schoolbook_quadform(schoolbook_gram(s, None, q, sign), c, q, sign, 2) == [_dot(z[0], z[0], q, sign)], (q, n)
        assert schoolbook_quadform(schoolbook_sym2(phi, s, q, sign), c, q, sign, 1) == [_dot(f[0], z[0], q, sign)], (q, n)
