"""Reference for the Galois automorphisms sigma_g: X -> X^g (lsr_ntt_ring_automorphism_batch), pure CPU, on Python
integers, in SCATTER form — the definition itself, not the gather form the kernels use:
    sigma_g(sum_i x_i X^i) = sum_i x_i X^(i g), with X^n = -1 (sign = -1: X^n + 1, N = 2 n) or X^n = 1 (sign = +1: X^n - 1, N = n).
The tests at the bottom (no GPU) pin it by hand."""


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
    from ring_tile_model import schoolbook
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
