"""References for the fused ring tile kernels (ring_mul, ring_dot, RingMatrix.matvec and matvec_gadget at n <= 4096), pure CPU.

Two references that share nothing with each other:
  * schoolbook*: the definition of the ring product on Python integers (sign = -1: X^n + 1, sign = +1: X^n - 1);
  * oracle_*:    the CPU oracle's transforms around a pointwise product.  Negacyclic: ntt_forward, mul_pointwise, ntt_inverse.  Cyclic:
                 cyclic_forward and cyclic_inverse with the pointwise products and sums in Python integers (Goldilocks lies above the
                 oracle's 2^61 pointwise limit).
The gadget digits come from ring_gadget_model.  The tests at the bottom (no GPU) hold the two references against each other in every
flavour of tests/test_ring_tile_sweep_gpu.py before either judges a kernel; that file re-exports them so that the suite collects them."""
from operator import mul

import numpy as np
import pytest

import ring_gadget_model as gadget
from ring_gadget_model import GOLDILOCKS, Q44, Q60

# flavour -> (modulus, cyclic ring X^n - 1).  The u64_q44 kernels are forced by lsr_set_arith_mode(1); the references are f64's.
FLAVOURS = {
    "f64": (Q44, False),
    "u64_q60": (Q60, False),
    "u64_q44": (Q44, False),
    "gold": (GOLDILOCKS, True),
    "cyc_f64": (Q44, True),
    "cyc_u64": (Q60, True),
}
GOLD_CARRY_POOL = (2**32 - 1, 2**32, 2**32 + 1, GOLDILOCKS - 2**32, 2**63, 2**63 + 1, 0xFFFFFFFF00000000)


# ---- the definition ---------------------------------------------------------------------------------------------------------------
def schoolbook(a, b, q, sign):
    """a * b mod (X^n - sign, q) as a list of Python integers (sign = -1: negacyclic).  Coefficient k is
    sum_{i <= k} a_i b_{k-i} + sign sum_{i > k} a_i b_{n+k-i}, each sum exact in Python integers and reduced once."""
    a, rb = [int(v) for v in a], [int(v) for v in b][::-1]
    n = len(a)
    return [(sum(map(mul, a[:k + 1], rb[n - 1 - k:])) + sign * sum(map(mul, a[k + 1:], rb[:n - 1 - k]))) % q for k in range(n)]


def schoolbook_dot(a, b, q, sign):
    """a: [batch][terms][n]; b: [batch][terms][n] or [terms][n] -> [batch][n] as nested lists."""
    out = []
    for j in range(a.shape[0]):
        bj = b if b.ndim == 2 else b[j]
        acc = [0] * a.shape[2]
        for i in range(a.shape[1]):
            acc = [(s + t) % q for s, t in zip(acc, schoolbook(a[j, i], bj[i], q, sign))]
        out.append(acc)
    return out


def schoolbook_matvec(m, x, q, sign):
    """m: [rows][cols][n]; x: [batch][cols][n] -> [batch][rows][n] as nested lists."""
    return [[schoolbook_dot(x[j:j + 1], m[r], q, sign)[0] for r in range(m.shape[0])] for j in range(x.shape[0])]


# ---- the oracle's transforms around a pointwise product ------------------------------------------------------------------------------
def root_of_order(q, n):
    """Some primitive n-th root of unity mod the prime q (n a power of two)."""
    g = 2
    while True:
        w = pow(g, (q - 1) // n, q)
        if n == 1 or pow(w, n // 2, q) == q - 1:
            return w
        g += 1


def _transform(oracle, q, n, polys, cyclic, omega, inverse=False):
    polys = np.ascontiguousarray(polys, dtype=np.uint64)
    if not cyclic:
        return (oracle.ntt_inverse if inverse else oracle.ntt_forward)(q, n, polys.reshape(-1, n)).reshape(polys.shape)
    fn = oracle.cyclic_inverse if inverse else oracle.cyclic_forward
    return np.stack([fn(row, q, omega) for row in polys.reshape(-1, n)]).reshape(polys.shape)


def _pointwise_sum(oracle, q, n, fa, fb, cyclic):
    """sum over axis -2 of fa * fb mod q (shapes equal: [..., terms, n]) -> [..., n] canonical uint64."""
    terms = fa.shape[-2]
    if cyclic:
        acc = 0
        for i in range(terms):
            acc = acc + fa[..., i, :].astype(object) * fb[..., i, :].astype(object)
        flat = [int(v) % q for v in np.ravel(acc)]
        return np.array(flat, dtype=np.uint64).reshape(fa.shape[:-2] + (n,))
    acc = np.zeros(fa.shape[:-2] + (n,), dtype=np.uint64)
    for i in range(terms):      # canonical summands: acc + prod < 2 q < 2^62
        prod = oracle.mul_pointwise(q, n, np.ascontiguousarray(fa[..., i, :]), np.ascontiguousarray(fb[..., i, :]))
        acc = acc + prod
        acc = acc - np.uint64(q) * (acc >= np.uint64(q)).astype(np.uint64)
    return acc


def oracle_dot(oracle, q, n, a, b, cyclic, omega):
    """a: [batch, terms, n]; b: [terms, n] (shared) or [batch, terms, n] -> [batch, n]: INTT(sum_i NTT(a_i) . NTT(b_i))."""
    fa = _transform(oracle, q, n, a, cyclic, omega)
    fb = np.broadcast_to(_transform(oracle, q, n, b, cyclic, omega), fa.shape)
    return _transform(oracle, q, n, _pointwise_sum(oracle, q, n, fa, fb, cyclic), cyclic, omega, inverse=True)


def oracle_product(oracle, q, n, a, b, cyclic, omega):
    """a: [batch, n]; b: [n] (shared) or [batch, n] -> [batch, n]."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    return oracle_dot(oracle, q, n, a[:, None, :], b[..., None, :], cyclic, omega)


def oracle_matvec(oracle, q, n, m, x, cyclic, omega):
    """m: [rows, cols, n]; x: [batch, cols, n] -> [batch, rows, n]."""
    rows, cols, batch = m.shape[0], m.shape[1], x.shape[0]
    fm = np.broadcast_to(_transform(oracle, q, n, m, cyclic, omega)[None], (batch, rows, cols, n))
    fx = np.broadcast_to(_transform(oracle, q, n, x, cyclic, omega)[:, None], (batch, rows, cols, n))
    return _transform(oracle, q, n, _pointwise_sum(oracle, q, n, fm, fx, cyclic), cyclic, omega, inverse=True)


def omega_for(oracle, flavour, n):
    """The root the flavour's cyclic context is created with (0 for the negacyclic flavours, whose oracle context has its own)."""
    q, cyclic = FLAVOURS[flavour]
    if not cyclic:
        return 0
    return oracle.prover_omega(n) if q == GOLDILOCKS else root_of_order(q, n)


# ---- operands -----------------------------------------------------------------------------------------------------------------------
def planted(rng, q, count, n):
    """[count, n] random residues with 0, 1, floor(q/2), floor(q/2) + 1, q - 2, q - 1 at the front of every element; for Goldilocks also
    the words around 2^32 and 2^63 that drive the carry and borrow paths of its reduction.  Where n is shorter than the list the
    elements cycle through it."""
    words = [0, 1, q // 2, q // 2 + 1, q - 2, q - 1]
    if q == GOLDILOCKS:
        words += [w % q for w in GOLD_CARRY_POOL]
    x = rng.integers(0, q, size=(count, n), dtype=np.uint64)
    front = min(n, len(words))
    for j in range(count):
        for k in range(front):
            x[j, k] = words[(j * front + k) % len(words)]
    return x


def goldilocks_lazy_carry(n):
    """A Goldilocks element (n >= 4) whose forward transform needs a lazy sum canonicalised: quarters (q/2 + 1, q/2, 2^63, 2^63).  The
    first stage pairs k with k + n/2 and leaves 2^64 - 2^31 + 1 and 2^64 - 2^31, both above q.  The second stage adds them: with the
    second operand reduced the sum wraps once to 2^32 - 1; unreduced it wraps twice and reads 0."""
    q, quarter = GOLDILOCKS, n // 4
    return np.array([q // 2 + 1] * quarter + [q // 2] * quarter + [2**63] * (2 * quarter), dtype=np.uint64)


def gadget_pairs(q):
    """(b, D, xcols): b = 11 and b = 4 at their minimum digit counts.  The 60-bit prime has no admissible D at b = 11 (5 digits are 55
    bits, 6 are 66 > 64): there b = 16 (D = 4) takes its place, and the sweep asserts the refusal of b = 11."""
    first = 11 if gadget.min_digits(q, 11) else 16
    assert gadget.min_digits(q, first) and gadget.min_digits(q, 4)
    return [(first, gadget.min_digits(q, first), 2), (4, gadget.min_digits(q, 4), 1)]


# ---- the two references agree (CPU only) ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 8, 64])
@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_schoolbook_equals_oracle_composition(oracle, flavour, n):
    (q, cyclic), omega = FLAVOURS[flavour], omega_for(oracle, flavour, n)
    sign = 1 if cyclic else -1
    rng = np.random.default_rng(n + len(flavour))
    batch, terms, rows, cols = 3, 3, 2, 3
    a, b = planted(rng, q, batch, n), planted(rng, q, batch, n)
    if cyclic and q == GOLDILOCKS and n >= 4:
        a[1] = b[1] = goldilocks_lazy_carry(n)
    assert oracle_product(oracle, q, n, a, b, cyclic, omega).tolist() == [schoolbook(a[j], b[j], q, sign) for j in range(batch)]
    assert oracle_product(oracle, q, n, a, b[2], cyclic, omega).tolist() == [schoolbook(a[j], b[2], q, sign) for j in range(batch)]
    da, db = planted(rng, q, batch * terms, n).reshape(batch, terms, n), planted(rng, q, batch * terms, n).reshape(batch, terms, n)
    assert oracle_dot(oracle, q, n, da, db, cyclic, omega).tolist() == schoolbook_dot(da, db, q, sign)
    assert oracle_dot(oracle, q, n, da, db[1], cyclic, omega).tolist() == schoolbook_dot(da, db[1], q, sign)
    m, x = planted(rng, q, rows * cols, n).reshape(rows, cols, n), planted(rng, q, batch * cols, n).reshape(batch, cols, n)
    m[1] = q - 1
    assert oracle_matvec(oracle, q, n, m, x, cyclic, omega).tolist() == schoolbook_matvec(m, x, q, sign)
    if q == GOLDILOCKS:
        assert not any(gadget.admissible(q, b, d) for b in range(2, 33) for d in range(1, 64 // b + 1))
        return
    for b, digits, xcols in gadget_pairs(q):
        gm = planted(rng, q, rows * xcols * digits, n).reshape(rows, xcols * digits, n)
        z = gadget.gadget_inverse(planted(rng, q, batch * xcols, n).reshape(batch, xcols, n), q, b, digits)
        assert oracle_matvec(oracle, q, n, gm, z, cyclic, omega).tolist() == schoolbook_matvec(gm, z, q, sign), (b, digits)


def test_schoolbook_by_hand():
    """(1 + 2X)(3 + 4X) = 3 + 10X + 8X^2: X^2 = -1 gives -5 + 10X, X^2 = 1 gives 11 + 10X."""
    assert schoolbook([1, 2], [3, 4], 97, -1) == [92, 10]
    assert schoolbook([1, 2], [3, 4], 97, 1) == [11, 10]
    assert schoolbook([0, 1, 0, 0], [0, 0, 0, 5], 97, -1) == [92, 0, 0, 0]


def test_planted_words_and_the_lazy_carry_element():
    rng = np.random.default_rng(0)
    for q in (Q44, Q60, GOLDILOCKS):
        x = planted(rng, q, 3, 16)
        assert int(x.max()) < q
        assert [int(v) for v in x[0, :6]] == [0, 1, q // 2, q // 2 + 1, q - 2, q - 1]
        seen = {int(v) for v in planted(rng, q, 13, 2).ravel()}
        assert {0, 1, q // 2, q // 2 + 1, q - 2, q - 1} <= seen
    assert [int(v) for v in planted(rng, GOLDILOCKS, 1, 16)[0, 6:13]] == [w % GOLDILOCKS for w in GOLD_CARRY_POOL]
    q, e = GOLDILOCKS, goldilocks_lazy_carry(8)
    first = [int(e[k]) + int(e[k + 4]) for k in range(4)]                 # the first stage's sums, as 64-bit words
    assert all(q <= s < 2**64 for s in first)
    assert first[0] + first[2] - 2**64 + 2**32 - 1 >= 2**64                # unreduced second operand: a second wrap
    assert first[0] + (first[2] - q) - 2**64 + 2**32 - 1 == 2**32 - 1     # reduced: 2^31 + (2^31 - 1)
