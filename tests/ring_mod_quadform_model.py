"""Model of the ring quadratic forms under an arbitrary modulus (lsr_ring_mod_quadform_*, batch.h "quadratic forms under any modulus",
DESIGN.md §5u) in Python integers on top of ring_mod_model.negacyclic_dot: no primes and no groups in the products.  It holds the
capacity of a cubic sum, the group rule, the status of a family, the form itself, and the exact integers the groups of a family sum to
over the centred operands (how close to the CRT range a test drives them).

A family of g is a nested list [r (r + 1) / 2][n] of words in the packed order of ring_mod_gram_model.index, a family of c is [r][n];
a batch is a list of families, and a shared c is a batch of one."""
import random

import ring_mod_gram_model as gram_model
import ring_mod_model as mod

SIZE_MAX = 2**64 - 1


def capacity_quadform(q, n, bound_g, bound_c):
    """floor(((P - 1) / 2) / (n^2 bound_g bound_c^2)), saturated at 2^64 - 1; a bound of 0 is floor(q / 2); 0 for a bound above
    floor(q / 2) and an inadmissible (q, n)"""
    h = q // 2
    if bound_g > h or bound_c > h or mod.capacity(q, n) == 0:
        return 0
    bound_g, bound_c = bound_g or h, bound_c or h
    p1, p2 = mod.primes(n)
    return min((p1 * p2 - 1) // 2 // (n * n * bound_g * bound_c * bound_c), SIZE_MAX)


def weight(q, offdiag):
    """what an off-diagonal pair costs: max(1, |w|) for the centred offdiag w"""
    return max(1, abs(mod.centre(offdiag, q)))


def groups(q, n, r, offdiag, bound_g=0, bound_c=0):
    """the sizes of the runs of the packed order the capacity alone cuts the r (r + 1) / 2 pairs into; [] where not one pair fits"""
    per = capacity_quadform(q, n, bound_g, bound_c) // weight(q, offdiag)
    if per == 0:
        return []
    pairs = r * (r + 1) // 2
    return [min(per, pairs - p0) for p0 in range(0, pairs, per)]


def _within(polys, q, bound):
    words = [int(w) for poly in polys for w in poly]
    if any(w >= q for w in words):
        return -1
    return 0 if any(abs(mod.centre(w, q)) > bound for w in words) else 1


def status(g_fam, c_fam, q, bound_g=0, bound_c=0):
    h = q // 2
    return min(_within(g_fam, q, bound_g or h), _within(c_fam, q, bound_c or h))


def quadform_family(g_fam, c_fam, q, offdiag):
    """sum_i c_i (g_ii c_i + offdiag sum_{l > i} g_il c_l) mod (X^n + 1, q), row by row"""
    r = len(c_fam)
    scaled = [[int(w) * offdiag % q for w in poly] for poly in c_fam]
    rows = [mod.negacyclic_dot([g_fam[gram_model.index(r, i, l)] for l in range(i, r)], [c_fam[i]] + scaled[i + 1:], q) for i in range(r)]
    return mod.negacyclic_dot(c_fam, rows, q)


def quadform(g, c, q, offdiag, bound_g=0, bound_c=0):
    """(out, status): out[j] is [n]; c holds one family per family of g, or one for all of them"""
    out, stats = [], []
    for j, g_fam in enumerate(g):
        c_fam = c[0] if len(c) == 1 else c[j]
        st = status(g_fam, c_fam, q, bound_g, bound_c)
        out.append(quadform_family(g_fam, c_fam, q, offdiag) if st == 1 else [0] * len(g_fam[0]))
        stats.append(st)
    return out, stats


def _integer_negacyclic(a, b):
    n = len(a)
    c = [0] * n
    for i, ai in enumerate(a):
        if ai:
            for j, bj in enumerate(b):
                if i + j < n:
                    c[i + j] += ai * bj
                else:
                    c[i + j - n] -= ai * bj
    return c


def group_magnitudes(g_fam, c_fam, q, offdiag, sizes):
    """the largest coefficient magnitude of the exact integer each group of `sizes` consecutive packed pairs sums to over the centred
    operands — what must stay within (P - 1) / 2"""
    r, n = len(c_fam), len(c_fam[0])
    cc = [[mod.centre(int(w), q) for w in poly] for poly in c_fam]
    w = mod.centre(offdiag, q)
    order = [(i, l) for i in range(r) for l in range(i, r)]
    out, p0 = [], 0
    for size in sizes:
        total = [0] * n
        for i, l in order[p0:p0 + size]:
            gg = [mod.centre(int(x), q) for x in g_fam[gram_model.index(r, i, l)]]
            term = _integer_negacyclic(gg, _integer_negacyclic(cc[i], cc[l]))
            total = [t + (1 if i == l else w) * v for t, v in zip(total, term)]
        out.append(max(abs(t) for t in total))
        p0 += size
    return out


def random_polys(rng, q, n, count, bound=0):
    if not bound:
        return [[rng.randrange(q) for _ in range(n)] for _ in range(count)]
    return [[rng.randint(-bound, bound) % q for _ in range(n)] for _ in range(count)]


# ---- the model's own tests (collected through tests/test_ring_mod_quadform_abi.py) -------------------------------------------------
CAPACITY_TABLE = [
    (4294967197, 64, 0, 2, 4398042366208),
    (4294967197, 64, 0, 1 << 20, 15),
    (4294967197, 64, 0, 1490944, 7),
    (4294967197, 64, 0, 0, 0),
    ((1 << 40) + 15, 64, 0, 2, 17179852592),
    ((1 << 40) + 15, 64, 128, 2, SIZE_MAX),
    (1 << 32, 4096, 0, 2, 1073740786),
    (1 << 32, 4096, 0, 0, 0),
    (1 << 32, 65536, 0, 2, 4194301),
    (3329, 256, 0, 0, 512471014808),
]


def test_model_capacity_quadform_table_zeros_and_the_group_rule():
    for q, n, bound_g, bound_c, want in CAPACITY_TABLE:
        assert capacity_quadform(q, n, bound_g, bound_c) == want, (q, n, bound_g, bound_c)
    for q, n in [(2, 2), (3329, 256), (4294967197, 64), (1 << 32, 8192)]:
        h = q // 2
        assert capacity_quadform(q, n, 0, 0) == capacity_quadform(q, n, h, h) == capacity_quadform(q, n, 0, h)
        assert capacity_quadform(q, n, h + 1, 1) == 0 == capacity_quadform(q, n, 1, h + 1)
        # one more operand within bound_c costs another n bound_c of the bilinear capacity
        for bound_g, bound_c in [(h, 1), (1, h), (h, h)]:
            bilinear = gram_model.capacity_product(q, n, bound_g, bound_c)
            if bilinear < SIZE_MAX:
                assert capacity_quadform(q, n, bound_g, bound_c) == bilinear // (n * bound_c)
    assert capacity_quadform(mod.largest_admissible(64) + 1, 64, 1, 1) == 0 and capacity_quadform(3329, 3, 1, 1) == 0
    q, n = 4294967197, 64
    assert weight(q, 2) == 2 and weight(q, 1) == 1 == weight(q, 0) == weight(q, q - 1) and weight(q, (q + 1) // 2) == q // 2
    assert groups(q, n, 7, 2, 0, 1490944) == [3] * 9 + [1] and groups(q, n, 7, 1, 0, 1490944) == [7] * 4
    assert groups(q, n, 7, q - 1, 0, 1490944) == [7] * 4 and groups(q, n, 7, 2) == []
    assert groups(q, n, 2, (q + 1) // 2, 0, 2) == [3] and groups(gram_model.Q40, n, 2, (gram_model.Q40 + 1) // 2, 0, 2) == []
    assert groups(3329, 256, 5, (3329 + 1) // 2) == [15] and capacity_quadform(3329, 256, 0, 0) // weight(3329, 1665) >= 15


def test_model_quadform_is_the_schoolbook_pair_by_pair_and_the_status_gates():
    rng = random.Random(37)
    for q, n, r, offdiag in [(3329, 4, 3, 2), (1 << 32, 16, 2, (1 << 32) - 1), (2, 8, 4, 1), (3, 2, 5, 2), ((1 << 40) + 15, 8, 3, 1)]:
        g = [random_polys(rng, q, n, r * (r + 1) // 2) for _ in range(2)]
        c = [random_polys(rng, q, n, r) for _ in range(2)]
        for j in range(2):
            want = [0] * n
            for i in range(r):
                for l in range(i, r):
                    term = mod.negacyclic_mul_schoolbook(g[j][gram_model.index(r, i, l)], mod.negacyclic_mul_schoolbook(c[j][i], c[j][l], q), q)
                    want = [(s + (1 if i == l else offdiag) * t) % q for s, t in zip(want, term)]
            assert quadform_family(g[j], c[j], q, offdiag) == want, (q, n, r)
        out, st = quadform(g, c, q, offdiag)
        assert st == [1, 1] and out[1] == quadform_family(g[1], c[1], q, offdiag)
        assert quadform(g, c[:1], q, offdiag)[0][1] == quadform_family(g[1], c[0], q, offdiag)          # one c for every family
    # status: the bounds are inclusive, -1 wins over 0, a gated family is all zeros; a bad word of a shared c gates every family
    q, n, r = 3329, 4, 2
    g = [random_polys(rng, q, n, 3, 9) for _ in range(3)]
    c = [random_polys(rng, q, n, 2, 2) for _ in range(3)]
    g[0][0][0], c[0][1][3] = 9, q - 2
    g[1][2][1] = q - 10
    c[2][0][0], g[2][1][1] = q, 10
    out, st = quadform(g, c, q, 2, 9, 2)
    assert st == [1, 0, -1] and any(out[0]) and not any(out[1]) and not any(out[2])
    assert quadform(g, c, q, 2, 10, 2)[1] == [1, 1, -1] and quadform(g, c, q, 2)[1] == [1, 1, -1]
    c[0][0][2] = 3
    assert quadform(g, c[:1], q, 2, 10, 2)[1] == [0, 0, 0] and quadform(g, c[:1], q, 2, 10, 3)[1] == [1, 1, 1]
    # the exact integers of the groups: the planted extreme reaches half of n^2 bound_g bound_c^2 per triple product
    h, beta = q // 2, 2
    flat = [[beta] * n] * 2
    signed = [[h if 2 * (n - 1 - a) + 2 - n > 0 else q - h for a in range(n)]] * 3
    assert group_magnitudes(signed, flat, q, 2, [3]) == [(1 + 2 + 1) * n * n * h * beta * beta // 2]
    assert group_magnitudes(signed, flat, q, q - 1, [1, 2]) == [n * n * h * beta * beta // 2, 0]
