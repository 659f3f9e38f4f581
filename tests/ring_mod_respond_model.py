"""Model of the masked response z = y + sum c s with its abort under an arbitrary modulus (lsr_ring_mod_respond_batch, batch.h
"responses under any modulus") in Python integers: ring_mod_model's negacyclic inner product (held against the
schoolbook product below), no primes and no groups of terms, and the status of an output with its precedence: -1 over 0 over 2 over 1.

v is a nested list [vectors][width][n] of words, p is [outputs][terms][n], y is [outputs][width][n] or None."""
import random

import ring_mod_fold_model as fold_model
import ring_mod_model as mod

REJECTED = 2


def _within(polys, q, bound):
    """1, 0 or -1 for the words of some polynomials"""
    words = [int(w) for poly in polys for w in poly]
    if any(w >= q for w in words):
        return -1
    return 0 if any(abs(mod.centre(w, q)) > bound for w in words) else 1


def respond(v, p, q, y=None, term_stride=0, bound_y=0, bound_v=0, bound_p=0, bound_z=0):
    """(out [outputs][width][n], status [outputs])"""
    h = q // 2
    bound_y, bound_v, bound_p, bound_z = bound_y or h, bound_v or h, bound_p or h, bound_z or h
    out, stats = [], []
    for j, challenges in enumerate(p):
        terms, n = len(challenges), len(challenges[0])
        vectors = [v[j * term_stride + i] for i in range(terms)]
        width = len(vectors[0])
        st = min(_within([poly for vec in vectors for poly in vec], q, bound_v), _within(challenges, q, bound_p))
        if y is not None:
            st = min(st, _within(y[j], q, bound_y))
        z = None
        if st == 1:
            z = []
            for c in range(width):
                acc = mod.negacyclic_dot([vec[c] for vec in vectors], challenges, q)
                if y is not None:
                    acc = [(s + int(t)) % q for s, t in zip(acc, y[j][c])]
                z.append(acc)
            if any(abs(mod.centre(w, q)) > bound_z for poly in z for w in poly):
                st = REJECTED
        out.append(z if st == 1 else [[0] * n for _ in range(width)])
        stats.append(st)
    return out, stats


# ---- the model's own tests (collected through tests/test_ring_mod_respond_abi.py) -------------------------------------------------
def test_model_response_is_the_fold_plus_the_mask():
    rng = random.Random(40)
    q, n, outputs, terms, width = 3329, 4, 3, 2, 2
    for stride in (0, 2, 1, 3):
        v = [fold_model.random_polys(rng, q, n, width) for _ in range((outputs - 1) * stride + terms)]
        p = [fold_model.random_polys(rng, q, n, terms) for _ in range(outputs)]
        y = [fold_model.random_polys(rng, q, n, width) for _ in range(outputs)]
        f, st = fold_model.fold(v, p, q, stride)
        assert respond(v, p, q, None, stride) == (f, st) and st == [1] * outputs
        z, st = respond(v, p, q, y, stride)
        assert st == [1] * outputs
        assert z == [[[(a + b) % q for a, b in zip(fp, yp)] for fp, yp in zip(fj, yj)] for fj, yj in zip(f, y)]
        for j in range(outputs):                                  # and word for word the schoolbook product
            for c in range(width):
                acc = list(y[j][c])
                for i in range(terms):
                    acc = [(s + t) % q for s, t in zip(acc, mod.negacyclic_mul_schoolbook(p[j][i], v[j * stride + i][c], q))]
                assert z[j][c] == acc, (stride, j, c)


def test_model_statuses_and_their_precedence():
    rng = random.Random(41)
    q, n, outputs, terms, width = 3329, 4, 3, 1, 2
    v = [fold_model.random_polys(rng, q, n, width, 2) for _ in range(outputs)]
    p = [fold_model.random_polys(rng, q, n, terms, 1) for _ in range(outputs)]
    f, _ = fold_model.fold(v, p, q, 1)
    bz = 100
    # the mask that puts every word of z at 0, then one word exactly at the bound, from either side: inclusive
    y = [[[(-w) % q for w in poly] for poly in fj] for fj in f]
    y[0][0][0] = (bz - f[0][0][0]) % q
    y[2][1][3] = (-bz - f[2][1][3]) % q
    z, st = respond(v, p, q, y, 1, 0, 2, 1, bz)
    assert st == [1, 1, 1] and z[0][0][0] == bz and z[2][1][3] == q - bz and sum(map(sum, z[1])) == 0
    y[1][1][3] = (-bz - 1 - f[1][1][3]) % q                  # one over, on the negative side: rejected, the neighbours intact
    z2, st = respond(v, p, q, y, 1, 0, 2, 1, bz)
    assert st == [1, REJECTED, 1] and z2[0] == z[0] and z2[2] == z[2] and not any(any(poly) for poly in z2[1])
    assert respond(v, p, q, y, 1, 0, 2, 1, 0)[1] == [1, 1, 1]                # bound_z = 0 never rejects
    by = q // 2 - 1
    y[1][0][0] = q // 2                                      # one over bound_y, the rejected word of z still in place
    assert respond(v, p, q, y, 1, by, 2, 1, bz)[1][1] == 0                  # 0 wins over 2
    y[1][0][1] = q
    z3, st = respond(v, p, q, y, 1, by, 2, 1, bz)
    assert st[1] == -1 and not any(any(poly) for poly in z3[1])             # -1 wins over 0
    v[1][0][0] = 3
    assert respond(v, p, q, None, 1, 0, 2, 1, bz)[1][1] == 0                # the fold's bounds, without a mask
