"""Model of the Gram matrices of bounded ring vectors under an arbitrary modulus (lsr_ring_mod_gram_*, batch.h "Gram matrices under any
modulus") in Python integers on top of ring_mod_model.negacyclic_dot: no primes and no column groups in the products —
an entry is the inner product of two vectors mod (X^n + 1, q) — the capacity with two short operands, and the status of a family.

A family is a nested list [vectors][width][n] of words; a batch is a list of families."""
import random

import ring_mod_model as mod

Q40 = (1 << 40) + 15


def capacity_product(q, n, bound_a, bound_b):
    """floor(((P - 1) / 2) / (n bound_a bound_b)), saturated at 2^64 - 1; 0 for a bound of 0 or above floor(q / 2) and an inadmissible (q, n)"""
    h = q // 2
    if bound_a == 0 or bound_b == 0 or bound_a > h or bound_b > h or mod.capacity(q, n) == 0:
        return 0
    p1, p2 = mod.primes(n)
    return min((p1 * p2 - 1) // 2 // (n * bound_a * bound_b), 2**64 - 1)


def index(r, i, l):
    """the polynomial of the pair i <= l in the packed upper triangle"""
    return i * r - i * (i - 1) // 2 + (l - i)


def _within(family, q, bound):
    """1, 0 or -1 for one operand of one family"""
    words = [int(w) for vec in family for poly in vec for w in poly]
    if any(w >= q for w in words):
        return -1
    return 0 if any(abs(mod.centre(w, q)) > bound for w in words) else 1


def status(a_fam, b_fam, q, bound_a=0, bound_b=0, b_is_a=False):
    """the status of one family: b_fam None — the symmetric form, which does not read bound_b; b_is_a — the cross form with b == a,
    whose words are held against both bounds"""
    h = q // 2
    bound_a, bound_b = bound_a or h, bound_b or h
    if b_fam is None:
        return _within(a_fam, q, bound_a)
    if b_is_a:
        bound_a = min(bound_a, bound_b)
    return min(_within(a_fam, q, bound_a), _within(b_fam, q, bound_b))


def _gated(entries, n, st):
    return entries if st == 1 else [[0] * n for _ in entries]


def gram(a, b, q, bound_a=0, bound_b=0):
    """(g, status): g[j] is [ra rb][n] (row-major), or for b None the packed upper triangle [r (r + 1) / 2][n]"""
    out, stats = [], []
    for j, a_fam in enumerate(a):
        n = len(a_fam[0][0])
        b_fam = None if b is None else b[j]
        st = status(a_fam, b_fam, q, bound_a, bound_b, b is a)
        if st != 1:
            count = len(a_fam) * (len(a_fam) + 1) // 2 if b is None else len(a_fam) * len(b_fam)
            entries = [[0] * n] * count
        elif b is None:
            entries = [mod.negacyclic_dot(a_fam[i], a_fam[l], q) for i in range(len(a_fam)) for l in range(i, len(a_fam))]
        else:
            entries = [mod.negacyclic_dot(x, y, q) for x in a_fam for y in b_fam]
        out.append(_gated(entries, n, st))
        stats.append(st)
    return out, stats


def gram_sym2(a, b, q, bound_a=0, bound_b=0):
    """(h, status): h[j] packed, <a_i, b_l> + <a_l, b_i> for i < l and <a_i, b_i> on the diagonal"""
    out, stats = [], []
    for a_fam, b_fam in zip(a, b):
        n, r = len(a_fam[0][0]), len(a_fam)
        st = status(a_fam, b_fam, q, bound_a, bound_b, b is a)
        entries = []
        for i in range(r):
            for l in range(i, r):
                if st != 1:
                    entries.append([0] * n)
                    continue
                first = mod.negacyclic_dot(a_fam[i], b_fam[l], q)
                if i == l:
                    entries.append(first)
                else:
                    entries.append([(u + v) % q for u, v in zip(first, mod.negacyclic_dot(a_fam[l], b_fam[i], q))])
        out.append(entries)
        stats.append(st)
    return out, stats


def random_family(rng, q, n, vectors, width, bound=0):
    """words whose centred representatives lie within `bound` (0: any word below q)"""
    if not bound:
        return [[[rng.randrange(q) for _ in range(n)] for _ in range(width)] for _ in range(vectors)]
    return [[[rng.randint(-bound, bound) % q for _ in range(n)] for _ in range(width)] for _ in range(vectors)]


# ---- the model's own tests (collected through tests/test_ring_mod_gram_abi.py) ----------------------------------------------------
def test_model_capacity_product_table_and_identities():
    p5 = mod.prime_5_mod_8_below(1 << 32)
    assert p5 == 4294967197
    table = {(Q40, 64): (7, 34359705185, 2**64 - 1, 2199021131904),
             (p5, 64): (524287, 8796084732416, 2**64 - 1, 2199021131904),
             (1 << 32, 4096): (8191, 137438820672, 2305840781199673368, 34359705168)}
    for (q, n), (full, one_short, both_short, wide) in table.items():
        h = q // 2
        assert capacity_product(q, n, h, h) == full == mod.capacity(q, n)
        assert capacity_product(q, n, h, 128) == one_short == capacity_product(q, n, 128, h)
        assert capacity_product(q, n, 128, 128) == both_short
        assert capacity_product(q, n, 1 << 20, 1 << 20) == wide
    for q, n in [(2, 2), (3329, 256), (Q40, 64), (1 << 32, 8192), (8246337208321, 8)]:
        h, pp = q // 2, mod.primes(n)
        assert capacity_product(q, n, h, h) == mod.capacity(q, n)
        for bound in (1, 2, h):
            if bound <= h:
                assert capacity_product(q, n, h, bound) == min((pp[0] * pp[1] - 1) // 2 // (n * h * bound), 2**64 - 1)      # capacity_bounded
        assert capacity_product(q, n, 0, h) == 0 == capacity_product(q, n, h, 0) == capacity_product(q, n, h + 1, 1) == capacity_product(q, n, 1, h + 1)
    assert mod.capacity(8246337208321, 8) == 1
    assert capacity_product(mod.largest_admissible(64) + 1, 64, 1, 1) == 0 and capacity_product(3329, 3, 1, 1) == 0


def test_model_gram_is_the_schoolbook_and_the_status_gates():
    rng = random.Random(34)
    q, n = 3329, 4
    a = [random_family(rng, q, n, 3, 2) for _ in range(2)]
    b = [random_family(rng, q, n, 2, 2) for _ in range(2)]

    def school(x, y):
        acc = [0] * n
        for u, v in zip(x, y):
            acc = [(s + t) % q for s, t in zip(acc, mod.negacyclic_mul_schoolbook(u, v, q))]
        return acc

    g, st = gram(a, b, q)
    assert st == [1, 1] and g[1][2 * 2 + 1] == school(a[1][2], b[1][1])
    s, st = gram(a, None, q)
    cross, _ = gram(a, a, q)
    assert st == [1, 1] and all(s[0][index(3, i, l)] == cross[0][i * 3 + l] for i in range(3) for l in range(i, 3))
    b3 = [random_family(rng, q, n, 3, 2) for _ in range(2)]
    h2, st = gram_sym2(a, b3, q)
    assert h2[0][index(3, 0, 2)] == [(u + v) % q for u, v in zip(school(a[0][0], b3[0][2]), school(a[0][2], b3[0][0]))]
    assert h2[0][index(3, 1, 1)] == school(a[0][1], b3[0][1])
    # status: the bound is inclusive, -1 wins over 0, a gated family is all zeros and its neighbours are not
    short = [random_family(rng, q, n, 3, 2, 5) for _ in range(3)]
    short[0][0][0][0], short[0][1][1][1] = 5, q - 5
    short[1][2][1][3] = 6
    short[2][0][0][0], short[2][1][0][0] = q, 6
    g, st = gram(short, None, q, 5)
    assert st == [1, 0, -1] and any(any(p) for p in g[0]) and not any(any(p) for p in g[1] + g[2])
    assert gram(short, None, q, 5, 1)[1] == [1, 0, -1]                    # the symmetric form does not read bound_b
    same, other = short[:1], [random_family(rng, q, n, 3, 2, 4)]
    assert gram(same, other, q, 5, 4)[1] == [1] and gram(other, same, q, 5, 4)[1] == [0]
    assert gram(same, same, q, 5, 4)[1] == [0] and gram(same, same, q, 5, 5)[1] == [1]     # b is a: held against both bounds
    assert status(short[0], short[0], q, 0, 0) == 1 and status(short[2], None, q) == -1
