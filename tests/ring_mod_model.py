"""Model of the ring handles under an arbitrary modulus (lsr_ring_mod_*, batch.h) in Python integers, independent of
the library: the two primes from its own Miller-Rabin search, the capacity, lift and reduce (CRT through pow(p1, -1, p2), not Garner
in 64-bit pieces), and the negacyclic product and inner product mod q.

`negacyclic_mul_schoolbook` is the definition.  `negacyclic_dot` computes the same sums through one big-integer product per term
(Kronecker substitution: exact integer arithmetic, no modular tricks), which is what keeps n = 256 affordable; the model's own tests
hold the two together."""
import functools
import random

DEFAULT_COMMIT_MODULUS = 17592169062401   # the default commitment modulus of every n <= 4096 (DESIGN.md "Commitment definition")
MAX_LOG2_N = 17


def is_prime(x):
    """Miller-Rabin with the first twelve primes as bases: deterministic below 3.3 * 10^24"""
    if x < 2:
        return False
    small = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    for p in small:
        if x % p == 0:
            return x == p
    d, s = x - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in small:
        y = pow(a, d, x)
        if y in (1, x - 1):
            continue
        for _ in range(s - 1):
            y = y * y % x
            if y == x - 1:
                break
        else:
            return False
    return True


def valid_degree(n):
    return 2 <= n <= 1 << MAX_LOG2_N and n & (n - 1) == 0


def _ntt_primes_44(n):
    """the 44-bit primes = 1 (mod 2n), largest first"""
    cand = ((1 << 44) - 1) // (2 * n) * (2 * n) + 1
    while cand > 1 << 43:
        if is_prime(cand):
            yield cand
        cand -= 2 * n


@functools.lru_cache(maxsize=None)
def primes(n):
    """(p1, p2): p1 the default commitment modulus for n — the fixed 44-bit prime up to n = 4096, the largest 44-bit prime
    = 1 (mod 2n) above — and p2 the largest 44-bit prime = 1 (mod 2n) other than p1.  None for an invalid n."""
    if not valid_degree(n):
        return None
    search = _ntt_primes_44(n)
    p1 = DEFAULT_COMMIT_MODULUS if n <= 4096 else next(search, None)
    if p1 is None:
        return None
    p2 = next((p for p in search if p != p1), None)
    return (p1, p2) if p2 is not None else None


def capacity(q, n):
    """max_terms = floor(((P - 1) / 2) / (n h^2)), h = floor(q / 2), saturated at 2^64 - 1 (a size_t); 0: not admissible"""
    pp = primes(n)
    if q < 2 or pp is None:
        return 0
    h = q // 2
    return min((pp[0] * pp[1] - 1) // 2 // (n * h * h), 2**64 - 1)


def centre(x, q):
    return x if x <= q // 2 else x - q


def lift(x, q, p):
    return centre(x, q) % p


def reduce(r0, r1, q, p1, p2):
    big = p1 * p2
    x = (r0 + p1 * ((r1 - r0) * pow(p1, -1, p2) % p2)) % big
    if x > (big - 1) // 2:
        x -= big
    return x % q


def residues(x, p1, p2):
    return x % p1, x % p2


def negacyclic_mul_schoolbook(a, b, q):
    n = len(a)
    c = [0] * n
    for i, ai in enumerate(a):
        ai = int(ai)
        for j, bj in enumerate(b):
            if i + j < n:
                c[i + j] += ai * int(bj)
            else:
                c[i + j - n] -= ai * int(bj)
    return [v % q for v in c]


def _pack(poly, slot_bytes):
    return int.from_bytes(b"".join(int(v).to_bytes(slot_bytes, "little") for v in poly), "little")


def negacyclic_dot(a_terms, b_terms, q):
    """sum_i a_i b_i mod (X^n + 1, q) for sequences of polynomials with coefficients in [0, q)"""
    n, terms = len(a_terms[0]), len(a_terms)
    slot_bytes = ((terms * n * (q - 1) ** 2).bit_length() + 8) // 8
    total = sum(_pack(a, slot_bytes) * _pack(b, slot_bytes) for a, b in zip(a_terms, b_terms))
    raw = total.to_bytes(2 * n * slot_bytes, "little")
    full = [int.from_bytes(raw[k * slot_bytes:(k + 1) * slot_bytes], "little") for k in range(2 * n)]
    return [(full[k] - full[k + n]) % q for k in range(n)]


def negacyclic_mul(a, b, q):
    return negacyclic_dot([a], [b], q)


def dot_coefficient(a_terms, b_terms, q, k):
    """coefficient k of sum_i a_i b_i mod (X^n + 1, q) as one row of the negacyclic matrix"""
    n, total = len(a_terms[0]), 0
    for a, b in zip(a_terms, b_terms):
        a, b = [int(v) for v in a], [int(v) for v in b]
        total += sum(a[i] * b[k - i] for i in range(k + 1)) - sum(a[i] * b[n + k - i] for i in range(k + 1, n))
    return total % q


def fold(z, c, q):
    """out[o][i] = sum_j c[o][j] z[j][i]: z [terms][width][n], c [outputs][terms][n] -> [outputs][width][n]"""
    return [[negacyclic_dot([c_o[j] for j in range(len(z))], [z[j][i] for j in range(len(z))], q) for i in range(len(z[0]))] for c_o in c]


def prime_5_mod_8_below(bound):
    """the largest prime = 5 (mod 8) below `bound`"""
    cand = bound - 1
    while not (cand % 8 == 5 and is_prime(cand)):
        cand -= 1
    return cand


def largest_admissible(n):
    """the largest q whose capacity at degree n is at least 1"""
    p1, p2 = primes(n)
    lo, hi = 2, 1 << 46
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if capacity(mid, n) >= 1 else (lo, mid)
    return lo


def edge_words(q):
    """the words at which lift and reduce decide: 0, 1, h = floor(q / 2) (the largest word that is its own centred representative),
    h + 1 (the most negative one; q - 1 at q = 2) and q - 1"""
    h = q // 2
    return [0, 1, h, min(h + 1, q - 1), q - 1]


def planted(rng, q, shape, fill=None):
    """A uint64 array [vectors, ..., n] of uniform words mod q (rng: a numpy Generator) with planted edges.
    fill {vector: word}: polynomial 0 of that vector is all `word` (the whole-polynomial extremes a caller pairs across two operands).
    The five edge_words sit at distinct random positions in every polynomial of vector 0 that `fill` leaves alone — as many of them as
    n holds, rotating through the five — and onward through the following free polynomials until each of the five has been planted."""
    import numpy as np
    fill = fill or {}
    n = shape[-1]
    x = rng.integers(0, q, size=shape, dtype=np.uint64)
    polys = x.reshape(shape[0], -1, n)
    per_vector, edges, take = polys.shape[1], edge_words(q), min(n, 5)
    nxt, done = 0, set()
    for k in range(shape[0] * per_vector):
        v, i = divmod(k, per_vector)
        if v >= 1 and len(done) == 5:
            break
        if i == 0 and v in fill:
            continue
        for pos in rng.choice(n, size=take, replace=False).tolist():
            polys[v, i, pos] = edges[nxt % 5]
            done.add(nxt % 5)
            nxt += 1
    for v, word in fill.items():
        polys[v, 0, :] = word
    if len(done) < 5:
        raise ValueError("shape %r is too small for the five edge words" % (shape,))
    return x


def dot_through_primes(a_terms, b_terms, q, centre=centre, reduce=reduce):
    """sum_i a_i b_i mod (X^n + 1, q) the way a handle computes it: the exact integer product of the centred operands (schoolbook),
    its residues mod the two primes, and reduce.  `centre` and `reduce` are arguments so that a test can hand in a broken copy."""
    n = len(a_terms[0])
    p1, p2 = primes(n)
    total = [0] * n
    for a, b in zip(a_terms, b_terms):
        a, b = [centre(int(v), q) for v in a], [centre(int(v), q) for v in b]
        for i, ai in enumerate(a):
            for j, bj in enumerate(b):
                if i + j < n:
                    total[i + j] += ai * bj
                else:
                    total[i + j - n] -= ai * bj
    return [reduce(*residues(v, p1, p2), q, p1, p2) for v in total]


# ---- the model's own tests (collected through tests/test_ring_mod_abi.py) --------------------------------------------------------
def test_kronecker_equals_schoolbook():
    rng = random.Random(5)
    for n, q in [(2, 2), (4, 3329), (16, (1 << 32)), (32, (1 << 40) + 15), (64, 3329)]:
        a = [[rng.randrange(q) for _ in range(n)] for _ in range(3)]
        b = [[rng.randrange(q) for _ in range(n)] for _ in range(3)]
        want = [0] * n
        for x, y in zip(a, b):
            want = [(w + v) % q for w, v in zip(want, negacyclic_mul_schoolbook(x, y, q))]
        assert negacyclic_dot(a, b, q) == want
        assert [dot_coefficient(a, b, q, k) for k in range(n)] == want
    a, b = [q - 1] * 64, [q - 1] * 64                        # the largest slots
    assert negacyclic_mul(a, b, q) == negacyclic_mul_schoolbook(a, b, q)


def test_primes_follow_the_rule():
    for n in [2, 64, 4096, 8192, 65536, 131072]:
        p1, p2 = primes(n)
        for p in (p1, p2):
            assert is_prime(p) and p % (2 * n) == 1 and 1 << 43 < p < 1 << 44
        assert p1 != p2
        top = next(_ntt_primes_44(n))
        assert p2 == top or p1 == top                          # nothing larger was skipped
    assert primes(3) is None and primes(1) is None and primes(1 << 18) is None


def test_lift_and_reduce_round_trip():
    p1, p2 = primes(64)
    big = p1 * p2
    for q in [2, 3, 3329, 1 << 32, (1 << 40) + 15]:
        for x in [0, 1, q // 2, min(q // 2 + 1, q - 1), q - 1]:
            assert reduce(lift(x, q, p1), lift(x, q, p2), q, p1, p2) == x
        for v in [0, 1, -1, (big - 1) // 2, -((big - 1) // 2), q, -q]:
            assert reduce(*residues(v, p1, p2), q, p1, p2) == v % q
    assert capacity(2, 64) == min((big - 1) // 2 // 64, 2**64 - 1) and capacity(1, 64) == 0 and capacity(3329, 3) == 0
    top = largest_admissible(64)
    assert capacity(top, 64) >= 1 and capacity(top + 1, 64) == 0


def test_planted_arrays_hold_the_five_edge_words():
    import numpy as np
    rng = np.random.default_rng(9)
    for n in (2, 4, 8, 64):
        for q in (largest_admissible(n), prime_5_mod_8_below(1 << 32), 3329):
            h, per_tile = q // 2, 4096 // n
            fill = {0: h, 1: h, per_tile: h, per_tile + 2: min(h + 1, q - 1)}
            for shape in [(per_tile + 3, n), (per_tile + 3, 3, n), (per_tile + 3, 2, 2, n)]:
                for f in ({}, fill):
                    x = planted(rng, q, shape, f)
                    assert x.shape == shape and x.dtype == np.uint64 and int(x.max()) < q
                    assert set(edge_words(q)) <= set(x.reshape(-1).tolist()), (n, q, shape)
                    polys = x.reshape(shape[0], -1, n)
                    for v, word in f.items():
                        assert (polys[v, 0] == word).all()
                    for i in range(polys.shape[1]):                                  # every free polynomial of vector 0 holds min(n, 5) of them
                        if not (i == 0 and 0 in f):
                            assert len(set(edge_words(q)) & set(polys[0, i].tolist())) >= min(n, 5), (n, q, i)
    assert edge_words(2) == [0, 1, 1, 1, 1] and edge_words(7) == [0, 1, 3, 4, 6]
    try:
        planted(rng, 3329, (1, 2), {0: 1})
    except ValueError:
        pass
    else:
        raise AssertionError("a shape without room for the five words is refused")


def test_planted_products_tell_broken_lift_and_reduce_apart():
    """Under the largest admissible q the planted pairs — all h by all h, and all h by all h + 1 (-h: that q is odd) — put n h^2 and
    -n h^2 into coefficient n - 1, within n (2 h + 1) of the ends of the CRT range.  A centre that sends h to h - q makes that
    coefficient n (h + 1)^2, outside the range: the reference changes.  The sign decision of reduce is pinned from both sides: a
    threshold n (2 h + 1) lower takes n h^2 for a negative, one as much higher takes -n h^2 for a positive.  `>` against `>=` differs
    at the integer (P - 1) / 2 alone, and no admissible operands produce it: a coefficient is at most n h^2 < (P - 1) / 2 in
    magnitude (asserted), so that one mistake is invisible through products — test_ring_mod_gpu.py's test_reduce_alone feeds the
    residues of (P - 1) / 2 themselves."""
    for n in (2, 4, 16):
        q = largest_admissible(n)
        h, (p1, p2) = q // 2, primes(n)
        half_p = (p1 * p2 - 1) // 2
        margin = n * (2 * h + 1)
        assert q % 2 == 1 and capacity(q, n) == 1 and capacity(q + 1, n) == 0
        assert 0 < half_p - n * h * h < margin
        pairs = [([h] * n, [h] * n), ([h] * n, [h + 1] * n)]

        def reference(centre_fn=centre, reduce_fn=reduce):
            return [dot_through_primes([a], [b], q, centre_fn, reduce_fn) for a, b in pairs]

        def reduce_with(threshold, strict=True):
            def broken(r0, r1, q_, p1_, p2_):
                big = p1_ * p2_
                x = (r0 + p1_ * ((r1 - r0) * pow(p1_, -1, p2_) % p2_)) % big
                if x > threshold or (not strict and x == threshold):
                    x -= big
                return x % q_
            return broken

        want = reference()
        assert want == [negacyclic_mul(a, b, q) for a, b in pairs]
        assert want[0][n - 1] == n * h * h % q and want[1][n - 1] == -n * h * h % q
        assert reference(reduce_fn=reduce_with(half_p)) == want                     # (the local copy is the model's reduce)
        assert reference(centre_fn=lambda x, q_: x if x < q_ // 2 else x - q_)[0] != want[0]
        assert reference(reduce_fn=reduce_with(half_p - margin))[0] != want[0]
        assert reference(reduce_fn=reduce_with(half_p + margin))[1] != want[1]
        assert reference(reduce_fn=reduce_with(half_p, strict=False)) == want       # >= : the same function on every admissible product
    rng = random.Random(11)
    for n, q in [(4, 3329), (8, largest_admissible(8)), (4, 1 << 32)]:
        a = [[rng.randrange(q) for _ in range(n)] for _ in range(1 if capacity(q, n) == 1 else 3)]
        b = [[rng.randrange(q) for _ in range(n)] for _ in a]
        assert dot_through_primes(a, b, q) == negacyclic_dot(a, b, q)
