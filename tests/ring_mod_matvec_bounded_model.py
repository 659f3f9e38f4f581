"""Model of the bounded resident-matrix product under an arbitrary modulus (lsr_ring_mod_matvec_bounded_batch, batch.h "resident
matrices under any modulus") in Python integers: ring_mod_matvec_model.matvec gated by ring_mod_fold_model's
within-bound rule.  Independent of the library: no primes, no groups in the product; `groups` states the grouping rule on its own."""
import random

import numpy as np

import ring_mod_fold_model as fold_model
import ring_mod_matvec_model as matvec_model

Q40 = fold_model.Q40


def matvec_bounded(m, x, q, bound=0):
    """m [rows][cols][n], x [batch][cols][n] -> (y [batch][rows][n] uint64, status [batch] int32): status[j] is 1 where every word of
    x[j] is below q and within `bound` (0: none, floor(q/2)) — then y[j] = M x[j] — 0 where one exceeds the bound, -1 where one is
    >= q (-1 wins); a gated y[j] is all zero"""
    m, x = np.asarray(m, dtype=np.uint64), np.asarray(x, dtype=np.uint64)
    bound = bound or q // 2
    status = np.array([fold_model._within(xj, q, bound) for xj in x.tolist()], dtype=np.int32)
    y = np.zeros((x.shape[0], m.shape[0], m.shape[2]), dtype=np.uint64)
    good = [j for j in range(x.shape[0]) if status[j] == 1]
    if good:
        y[good] = matvec_model.matvec(m, x[good], q)
    return y, status


def groups(q, n, cols, bound=0):
    """the sizes of the groups of matrix columns a call takes under this bound (0: none)"""
    capacity = matvec_model.capacity_bounded(q, n, bound or q // 2)
    return [min(capacity, cols - c0) for c0 in range(0, cols, capacity)]


# ---- the model's own tests (collected through tests/test_ring_mod_matvec_bounded_abi.py) -------------------------------------------
def test_model_matvec_bounded_gates_whole_vectors():
    rng = random.Random(38)
    q, n, rows, cols, bound = 3329, 4, 2, 3, 5
    m = [fold_model.random_polys(rng, q, n, cols) for _ in range(rows)]
    x = [fold_model.random_polys(rng, q, n, cols, bound) for _ in range(5)]
    x[0][0][0], x[0][2][3] = bound, q - bound                      # met exactly, from both sides
    x[1][2][3] = bound + 1
    x[2][0][1] = q - bound - 1
    x[3][1][0], x[3][1][1] = bound + 1, q                          # -1 wins over 0
    y, status = matvec_bounded(m, x, q, bound)
    assert status.tolist() == [1, 0, 0, -1, 1]
    plain = matvec_model.matvec(m, np.array(x, dtype=np.uint64) % q, q)
    for j in range(5):
        assert np.array_equal(y[j], plain[j]) if status[j] == 1 else not y[j].any()
    y0, status0 = matvec_bounded(m, x, q)                          # no bound: only -1 can occur
    assert status0.tolist() == [1, 1, 1, -1, 1] and np.array_equal(y0[[0, 1, 2, 4]], plain[[0, 1, 2, 4]]) and not y0[3].any()
    assert np.array_equal(matvec_bounded(m, x, q, q // 2)[0], y0)


def test_model_groups():
    q, n, h = Q40, 64, Q40 // 2
    assert groups(q, n, 50) == [7] * 7 + [1] and len(groups(q, n, 50)) == 8
    assert matvec_model.capacity_bounded(q, n, h // 3) == 23 and groups(q, n, 50, h // 3) == [23, 23, 4]
    assert groups(q, n, 50, 128) == [50] and groups(q, n, 258, 128) == [258] and len(groups(q, n, 258)) == 37
    assert groups(q, n, 50, h) == groups(q, n, 50)
