"""Reference for the Galois automorphisms sigma_g: X -> X^g (lsr_ntt_ring_automorphism_batch), pure CPU, on Python
integers, in SCATTER form — the definition itself, not the gather form the kernels use:
    sigma_g(sum_i x_i X^i) = sum_i x_i X^(i g), with X^n = -1 (sign = -1: X^n + 1, N = 2 n) or X^n = 1 (sign = +1: X^n - 1, N = n).
automorphism_np is the same scatter vectorised for the 2^17-word cases, galois_dot_ref the reference of the twisted inner product.
The tests at the bottom (no GPU) pin the list model by hand, the vectorised one against it, and galois_dot_ref and
ring_fold_model.fold_ref against the schoolbook."""
import numpy as np
import pytest

from ring_tile_model import FLAVOURS, GOLDILOCKS, goldilocks_lazy_carry, omega_for, oracle_dot, planted, schoolbook, schoolbook_dot


def galois_order(n, sign):
    """N: the order of X in the ring."""
    return 2 * n if sign < 0 else n


def galois_elements(n, sign):
    return list(range(1, galois_order(n, sign), 2))


def automorphism(x, g, q, sign):
    """sigma_g of one ring element x (a sequence of n canonical words) as a list of Python integers."""
    n, order = len(x), galois_order(len(x), sign)
    assert g % 2 == 1 and 1 <= g < order
    out = [0] * n
    for i, word in enumerate(x):
        e = i * g % order                    # X^(i g) = X^e, e < N
        if e < n:
            out[e] = (out[e] + int(word)) % q
        else:                                # (negacyclic only) X^e = -X^(e - n)
            out[e - n] = (out[e - n] - int(word)) % q
    return out


def automorphism_batch(x, g, q, sign):
    """x: [..., n] nested -> the same nesting with sigma_g applied to every innermost element."""
    if len(x) and hasattr(x[0], "__len__"):
        return [automorphism_batch(e, g, q, sign) for e in x]
    return automorphism(x, g, q, sign)


def automorphism_np(x, g, q, sign):
    """sigma_g of every element of x [..., n] (canonical uint64 words), vectorised, still in scatter form: destination index and sign
    of source word i from i g mod N, then one assignment — g is odd and N a power of two, so i -> i g mod N is a permutation and no
    destination receives two words (the list model's additions are assignments)."""
    x = np.asarray(x, dtype=np.uint64)
    n, order = x.shape[-1], galois_order(x.shape[-1], sign)
    assert g % 2 == 1 and 1 <= g < order and n & (n - 1) == 0
    e = (np.arange(n, dtype=np.uint64) * np.uint64(g)) % np.uint64(order)          # i g < 2^64 by far
    dest, negated = e % np.uint64(n), e >= np.uint64(n)
    assert len(np.unique(dest)) == n
    out = np.empty_like(x)
    out[..., dest.astype(np.intp)] = np.where(negated & (x != 0), np.uint64(q) - x, x)      # -0 = 0; q - x stays inside uint64
    return out


def galois_dot_ref(oracle, q, n, a, b, g, cyclic, omega):
    """sum_i sigma_g(a_i) b_i: ring_tile_model.oracle_dot on the scattered a.  Shapes as oracle_dot."""
    return oracle_dot(oracle, q, n, automorphism_np(a, g, q, 1 if cyclic else -1), b, cyclic, omega)


# ---- by hand (CPU only) --------------------------------------------------------------------------------------------------------------
def test_automorphism_by_hand():
    q = 97
    x = [1, 2, 3, 4]                                              # 1 + 2 X + 3 X^2 + 4 X^3
    # X^4 + 1, g = 3: X -> X^3, X^2 -> X^6 = -X^2, X^3 -> X^9 = X
    assert automorphism(x, 3, q, -1) == [1, 4, q - 3, 2]
    # g = 7 = N - 1 (conjugation): X -> X^7 = -X^3, X^2 -> X^14 = -X^2, X^3 -> X^21 = X^5 = -X
    assert automorphism(x, 7, q, -1) == [1, q - 4, q - 3, q - 2]
    assert automorphism(x, 1, q, -1) == x
    # X^4 - 1, g = 3 = N - 1: X -> X^3, X^2 -> X^6 = X^2, X^3 -> X^9 = X
    assert automorphism(x, 3, q, 1) == [1, 4, 3, 2]
    assert automorphism([0, 0, 5, 0], 3, q, -1) == [0, 0, q - 5, 0]
    assert galois_elements(4, -1) == [1, 3, 5, 7] and galois_elements(4, 1) == [1, 3] and galois_elements(2, 1) == [1]


def test_automorphism_is_a_ring_homomorphism_and_a_group_action():
    q, n = 97, 8
    a, b = [3, 1, 4, 1, 5, 9, 2, 6], [2, 7, 1, 8, 2, 8, 1, 8]
    for sign in (-1, 1):
        order = galois_order(n, sign)

        def mul(u, v):
            return schoolbook(u, v, q, sign)

        for g in galois_elements(n, sign):
            assert automorphism(mul(a, b), g, q, sign) == mul(automorphism(a, g, q, sign), automorphism(b, g, q, sign)), (sign, g)
            for h in galois_elements(n, sign):
                assert automorphism(automorphism(a, h, q, sign), g, q, sign) == automorphism(a, g * h % order, q, sign), (sign, g, h)
        # the constant term of conj(a) b is the inner product of the coefficient vectors
        assert mul(automorphism(a, order - 1, q, sign), b)[0] == sum(x * y for x, y in zip(a, b)) % q


# ---- the vectorised scatter equals the list model; the two new references equal the schoolbook (CPU only) --------------------------------
def test_automorphism_np_equals_the_list_model():
    rng = np.random.default_rng(43)
    for q in (97, GOLDILOCKS):
        for sign in (-1, 1):
            for n in (2, 4, 8, 16):
                x = rng.integers(0, q, size=(3, n), dtype=np.uint64)
                x[0, :2] = [0, q - 1]
                x[1] = q - 1
                x[2, n - 1] = 0
                for g in galois_elements(n, sign):
                    assert automorphism_np(x, g, q, sign).tolist() == automorphism_batch(x.tolist(), g, q, sign), (q, sign, n, g)
            n = 4096
            order = galois_order(n, sign)
            x = planted(rng, q, 2, n)                       # 0 and q - 1 among the planted words
            x[1, n - 2:] = [q - 1, 0]
            for g in (3, order - 1, order // 2 + 1, order - 5):
                assert automorphism_np(x, g, q, sign).tolist() == automorphism_batch(x.tolist(), g, q, sign), (q, sign, n, g)
            assert automorphism_np(x.reshape(2, 1, n), 3, q, sign).shape == (2, 1, n)            # [..., n] keeps its shape


@pytest.mark.parametrize("n", [2, 8, 64])
@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_references_equal_the_schoolbook(oracle, flavour, n):
    """galois_dot_ref against schoolbook_dot on the list model's sigma_g(a), ring_fold_model.fold_ref against schoolbook_fold, in every
    flavour of the tile sweeps, before either reference judges a kernel."""
    from ring_fold_model import fold_ref, schoolbook_fold, vectors_needed
    (q, cyclic), omega = FLAVOURS[flavour], omega_for(oracle, flavour, n)
    sign = 1 if cyclic else -1
    rng = np.random.default_rng(7 * n + len(flavour))
    lazy = goldilocks_lazy_carry(n) if q == GOLDILOCKS and n >= 4 else None
    batch, terms = 3, 3
    a, b = planted(rng, q, batch * terms, n).reshape(batch, terms, n), planted(rng, q, batch * terms, n).reshape(batch, terms, n)
    if lazy is not None:
        a[1, 0] = b[1, 2] = b[2, 1] = lazy
    for g in galois_elements(n, sign) if n <= 8 else (1, 3, galois_order(n, sign) // 2 + 1, galois_order(n, sign) - 5, galois_order(n, sign) - 1):
        sa = np.array(automorphism_batch(a.tolist(), g, q, sign), dtype=np.uint64)
        assert galois_dot_ref(oracle, q, n, a, b, g, cyclic, omega).tolist() == schoolbook_dot(sa, b, q, sign), (flavour, n, g)
        assert galois_dot_ref(oracle, q, n, a, b[2], g, cyclic, omega).tolist() == schoolbook_dot(sa, b[2], q, sign), (flavour, n, g, "shared b")
    outputs, width = 2, 3
    for stride in (0, 1, terms):
        v = planted(rng, q, vectors_needed(outputs, terms, stride) * width, n).reshape(-1, width, n)
        p = planted(rng, q, outputs * terms, n).reshape(outputs, terms, n)
        if lazy is not None:
            v[1, 1] = p[1, 2] = lazy
        assert fold_ref(oracle, q, n, v, p, stride, cyclic, omega).tolist() == schoolbook_fold(v, p, stride, q, sign), (flavour, n, stride)
