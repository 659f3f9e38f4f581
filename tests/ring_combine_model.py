"""Model of the ring-element linear combination of commitment rows: what lsr_lwe_ring_combine_rows_device must
compute, independently of any kernel.

    out = sum_i p'_i(X) * row_i      component by component in Z_q[X]/(X^n + 1),  p'_i = the centred coefficients of polys[i] mod t

Two forms of the negacyclic product of a canonical residue array with a signed polynomial:
  * sparse: X^x * a is a rotation with a sign flip of the wrapped part, so p' * a is a sum of signed shifted copies of a, one per
    non-zero coefficient.  The sums are exact integers: the residues are split into 32-bit limbs and each limb's signed sum is kept in
    int64 (asserted to fit), then recombined and reduced mod q in Python integers;
  * dense: through the oracle's transforms, INTT(sum_i NTT(a_i) . NTT(p'_i mod q)), the sum taken mod q in Python integers (the way
    tests/test_ring_dot_gpu.py builds its expectation).
Row assembly reuses combine_model (centring, weight, default rows) and rns_model (the RNS header)."""
import numpy as np

import combine_model
import rns_model


def centred_poly(words, t):
    """the centred representatives of the coefficient words mod t, as int64"""
    return np.array([combine_model.centred(int(c), t) for c in np.ravel(words)], dtype=np.int64)


def centred_words(words, t):
    """centred_poly in the shape of `words` and without the Python loop (t < 2^63), for the calls of many thousand terms"""
    c = np.asarray(words, dtype=np.uint64) % np.uint64(t)
    return np.where(c > np.uint64(t // 2), c.astype(np.int64) - np.int64(t), c.astype(np.int64))


def weight(polys, t):
    """sum over every coefficient of every polynomial of |c'|: what the budget is compared with"""
    return combine_model.weight(np.ravel(polys), t)


def fold_shared_rows(polys, row_of_term, distinct, t):
    """Terms that share a row: sum_i p'_i * row[r(i)] = sum_r (sum_{i : r(i) = r} p'_i) * row[r].  polys: uint64 [terms][n] words,
    row_of_term: [terms] indices below `distinct` -> uint64 [distinct][n] words whose centred representatives are the inner sums
    (asserted to lie within (-t/2, t/2], so that centring returns them)."""
    sums = np.zeros((distinct, polys.shape[1]), dtype=np.int64)
    np.add.at(sums, np.asarray(row_of_term), centred_words(polys, t))
    assert int(np.abs(sums).max()) < t // 2, "the folded coefficients leave the centred range"
    return np.where(sums < 0, sums + np.int64(t), sums).astype(np.uint64)


def layout(n, k, moduli):
    """(header words, [(first word, words, modulus)]) of a row under one modulus (default, wide) or two (RNS)"""
    head = 6 if len(moduli) == 2 else 5
    block = (k + 1) * n
    return head, [(head + i * block, block, int(q)) for i, q in enumerate(moduli)]


def _shifted(a, x):
    """X^x * a for 0 <= x < len(a), a int64"""
    return a if x == 0 else np.concatenate((-a[len(a) - x:], a[:len(a) - x]))


def dot_sparse(residues, polys, q):
    """sum_i polys[i] * residues[i] mod (X^n + 1, q); residues: uint64 [terms][n] canonical, polys: int64 [terms][n] centred"""
    n = residues.shape[1]
    lo_sum, hi_sum = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    bound = 0
    for a, p in zip(residues, polys):
        lo, hi = (a & np.uint64(0xFFFFFFFF)).astype(np.int64), (a >> np.uint64(32)).astype(np.int64)
        for x in np.flatnonzero(p):
            c = int(p[x])
            bound += abs(c) << 32
            lo_sum += c * _shifted(lo, int(x))
            hi_sum += c * _shifted(hi, int(x))
    assert bound < 2**62, "too many taps for the int64 limb sums: use dot_dense"
    total = hi_sum.astype(object) * (1 << 32) + lo_sum.astype(object)
    return np.array([int(v) % q for v in total], dtype=np.uint64)


def dot_schoolbook(residues, polys, q):
    """the same by the definition, on Python integers: coefficient x + y of the product receives p[x] a[y], negated past X^n"""
    n = residues.shape[1]
    acc = [0] * n
    for a, p in zip(residues, polys):
        a = [int(v) for v in a]
        for x, c in enumerate(int(c) for c in p):
            if c == 0:
                continue
            for y, v in enumerate(a):
                if x + y < n:
                    acc[x + y] += c * v
                else:
                    acc[x + y - n] -= c * v
    return np.array([v % q for v in acc], dtype=np.uint64)


def dot_dense(oracle, residues, polys, q):
    """the same through the oracle's negacyclic transforms"""
    n = residues.shape[1]
    lifted = np.array([[int(c) % q for c in p] for p in polys], dtype=np.uint64)
    fa = oracle.ntt_forward(q, n, np.ascontiguousarray(residues))
    fp = oracle.ntt_forward(q, n, lifted)
    prod = np.asarray(oracle.mul_pointwise(q, n, fa, fp)).reshape(len(polys), n).astype(object)
    summed = np.array([int(v) for v in prod.sum(axis=0) % q], dtype=np.uint64).reshape(1, n)
    return np.asarray(oracle.ntt_inverse(q, n, summed)).reshape(n)


def combine_row(rows, polys, t, n, k, moduli, oracle=None, schoolbook=False):
    """wire rows (uint64 [terms][words]) and coefficient words (uint64 [terms][n]) -> the combined row (uint64 [words]); the dense form
    when an oracle is given, the schoolbook when asked for, the sparse form otherwise"""
    head, blocks = layout(n, k, moduli)
    centred = np.array([centred_poly(p, t) for p in polys])
    out = np.zeros(rows.shape[1], dtype=np.uint64)
    out[:head] = rows[0][:head]
    for first, _, q in blocks:
        for c in range(k + 1):
            lo = first + c * n
            comp = np.ascontiguousarray(rows[:, lo:lo + n])
            if schoolbook:
                out[lo:lo + n] = dot_schoolbook(comp, centred, q)
            else:
                out[lo:lo + n] = dot_dense(oracle, comp, centred, q) if oracle is not None else dot_sparse(comp, centred, q)
    return out


def combine_rows(rows, polys, term_stride, t, n, k, moduli, oracle=None, schoolbook=False):
    """the whole call: polys uint64 [outputs][terms][n] -> uint64 [outputs][words]"""
    outputs, terms = polys.shape[:2]
    return np.array([combine_row(rows[j * term_stride:j * term_stride + terms], polys[j], t, n, k, moduli, oracle, schoolbook)
                     for j in range(outputs)])


def message(msgs, polys, t):
    """what a combined row opens to: sum_i p'_i * m_i mod (X^n + 1, t); msgs uint64 [terms][n] (all n slots)"""
    return dot_sparse(np.ascontiguousarray(msgs, dtype=np.uint64), np.array([centred_poly(p, t) for p in polys]), t)


def rns_header(n, k, t, moduli):
    return rns_model.header(n, k, t, int(moduli[0]), int(moduli[1]))
