"""Model of the fold of ring vectors by ring-valued challenges under an arbitrary modulus (lsr_ring_mod_fold_batch, batch.h "fold under
any modulus") in Python integers on top of ring_mod_model.negacyclic_dot and ring_mod_gram_model.capacity_product: no
primes and no groups of terms — an output polynomial is the inner product of its gathered operands mod (X^n + 1, q) — and the status
of an output.

v is a nested list [vectors][width][n] of words, p is [outputs][terms][n]."""
import random

import ring_mod_gram_model as gram_model
import ring_mod_model as mod

Q40 = gram_model.Q40


def groups(q, n, terms, bound_v=0, bound_p=0):
    """the sizes of the groups of terms a call takes under these bounds (0: none)"""
    h = q // 2
    capacity = gram_model.capacity_product(q, n, bound_v or h, bound_p or h)
    return [min(capacity, terms - i0) for i0 in range(0, terms, capacity)]


def _within(polys, q, bound):
    """1, 0 or -1 for the words of some polynomials"""
    words = [int(w) for poly in polys for w in poly]
    if any(w >= q for w in words):
        return -1
    return 0 if any(abs(mod.centre(w, q)) > bound for w in words) else 1


def fold(v, p, q, term_stride=0, bound_v=0, bound_p=0):
    """(out [outputs][width][n], status [outputs])"""
    h = q // 2
    bound_v, bound_p = bound_v or h, bound_p or h
    out, stats = [], []
    for j, challenges in enumerate(p):
        terms, n = len(challenges), len(challenges[0])
        vectors = [v[j * term_stride + i] for i in range(terms)]
        width = len(vectors[0])
        st = min(_within([poly for vec in vectors for poly in vec], q, bound_v), _within(challenges, q, bound_p))
        if st == 1:
            out.append([mod.negacyclic_dot([vec[c] for vec in vectors], challenges, q) for c in range(width)])
        else:
            out.append([[0] * n for _ in range(width)])
        stats.append(st)
    return out, stats


def random_polys(rng, q, n, count, bound=0):
    """[count][n] words whose centred representatives lie within `bound` (0: any word below q)"""
    if not bound:
        return [[rng.randrange(q) for _ in range(n)] for _ in range(count)]
    return [[rng.randint(-bound, bound) % q for _ in range(n)] for _ in range(count)]


# ---- the model's own tests (collected through tests/test_ring_mod_fold_abi.py) ----------------------------------------------------
def test_model_fold_is_the_schoolbook_at_every_stride():
    rng = random.Random(35)
    q, n, outputs, terms, width = 3329, 4, 3, 2, 2
    for stride in (0, 2, 1, 3):
        vectors = (outputs - 1) * stride + terms
        v = [random_polys(rng, q, n, width) for _ in range(vectors)]
        p = [random_polys(rng, q, n, terms) for _ in range(outputs)]
        out, st = fold(v, p, q, stride)
        assert st == [1] * outputs
        for j in range(outputs):
            for c in range(width):
                acc = [0] * n
                for i in range(terms):
                    acc = [(s + t) % q for s, t in zip(acc, mod.negacyclic_mul_schoolbook(p[j][i], v[j * stride + i][c], q))]
                assert out[j][c] == acc, (stride, j, c)
    # one output from a 2-d view of the same data is ring_mod_model.fold
    assert fold(v[:terms], p[:1], q, 0)[0] == mod.fold(v[:terms], p[:1], q)


def test_model_status_gates_and_groups():
    rng = random.Random(36)
    q, n, outputs, terms, width = 3329, 4, 3, 2, 2
    v = [random_polys(rng, q, n, width, 5) for _ in range(outputs * terms)]
    p = [random_polys(rng, q, n, terms, 2) for _ in range(outputs)]
    v[0][0][0], v[1][1][3] = 5, q - 5                       # the bound is inclusive on both sides
    p[0][0][0], p[0][1][1] = 2, q - 2
    assert fold(v, p, q, terms, 5, 2)[1] == [1, 1, 1]
    v[2][1][2] = 6                                          # output 1 reads vectors 2 and 3
    out, st = fold(v, p, q, terms, 5, 2)
    assert st == [1, 0, 1] and not any(any(poly) for poly in out[1]) and any(any(poly) for poly in out[0] + out[2])
    p[2][0][0] = q - 3
    assert fold(v, p, q, terms, 5, 2)[1] == [1, 0, 0]
    p[2][1][0] = q                                          # -1 wins over 0
    assert fold(v, p, q, terms, 5, 2)[1] == [1, 0, -1]
    assert fold(v, p, q, terms)[1] == [1, 1, -1]            # no bounds: only the range is held
    # shared terms: a bad word of v gates every output, a bad word of p[j] gates j alone
    shared = [random_polys(rng, q, n, width, 5) for _ in range(terms)]
    p = [random_polys(rng, q, n, terms, 2) for _ in range(outputs)]
    p[1][0][0] = 3
    assert fold(shared, p, q, 0, 5, 2)[1] == [1, 0, 1]
    shared[1][0][0] = q - 6
    assert fold(shared, p, q, 0, 5, 2)[1] == [0, 0, 0]
    # the groups a call takes: the capacities batch.h quotes
    h = Q40 // 2
    assert groups(Q40, 64, 9) == [7, 2] and groups(Q40, 64, 9, 0, 2) == [9] and groups(Q40, 64, 16, 0, h // 2) == [15, 1]
    assert gram_model.capacity_product(Q40, 64, h, 2) == 2199021131876
    assert groups(mod.largest_admissible(64), 64, 3) == [1, 1, 1]
