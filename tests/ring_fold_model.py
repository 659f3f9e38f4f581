"""References for the fold of ring vectors by ring-valued challenges (lsr_ntt_ring_fold_batch), pure CPU:
out[j][c] = sum_{i < terms} p[j][i] * v[j term_stride + i][c].

  * gather:          the ring-dot operands the fold is defined by — a[(j, c)][i] = v[j term_stride + i][c], b[(j, c)][i] = p[j][i];
  * schoolbook_fold: the definition on Python integers, through ring_tile_model.schoolbook_dot on the gathered operands;
  * fold_ref:        the oracle's composition INTT(sum NTT . NTT) on the gathered operands, for the sizes the schoolbook is too slow at.
The tests at the bottom (no GPU) pin the gather by hand; ring_galois_model.test_references_equal_the_schoolbook holds fold_ref against
schoolbook_fold."""
import numpy as np

from ring_tile_model import oracle_dot, schoolbook_dot


def vectors_needed(outputs, terms, term_stride):
    return (outputs - 1) * term_stride + terms


def gather(v, p, term_stride):
    """v: [vectors, width, n]; p: [outputs, terms, n] -> (a, b), each [outputs * width, terms, n], output (j, c) at row j width + c."""
    v, p = np.asarray(v, dtype=np.uint64), np.asarray(p, dtype=np.uint64)
    outputs, terms, n = p.shape
    width = v.shape[1]
    assert v.shape[0] >= vectors_needed(outputs, terms, term_stride) and v.shape[2] == n
    rows = np.arange(outputs)[:, None] * term_stride + np.arange(terms)[None, :]          # [outputs, terms]
    a = v[rows].transpose(0, 2, 1, 3).reshape(outputs * width, terms, n)                   # [outputs, width, terms, n]
    b = np.broadcast_to(p[:, None], (outputs, width, terms, n)).reshape(outputs * width, terms, n)
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def schoolbook_fold(v, p, term_stride, q, sign):
    """[outputs][width][n] as nested lists of Python integers (sign = -1: X^n + 1, +1: X^n - 1)."""
    outputs, width = p.shape[0], v.shape[1]
    a, b = gather(v, p, term_stride)
    flat = schoolbook_dot(a, b, q, sign)
    return [flat[j * width:(j + 1) * width] for j in range(outputs)]


def fold_ref(oracle, q, n, v, p, term_stride, cyclic, omega):
    """[outputs, width, n] uint64: ring_tile_model.oracle_dot (the oracle's transforms around pointwise sums) on the gathered
    operands."""
    a, b = gather(v, p, term_stride)
    return oracle_dot(oracle, q, n, a, b, cyclic, omega).reshape(p.shape[0], v.shape[1], n)


# ---- the gather by hand (CPU only) ---------------------------------------------------------------------------------------------------
def test_gather_by_hand():
    n, width, terms, outputs = 2, 2, 2, 2
    v = np.arange(4 * width * n, dtype=np.uint64).reshape(4, width, n)
    p = 100 + np.arange(outputs * terms * n, dtype=np.uint64).reshape(outputs, terms, n)
    for stride, rows in [(0, [[0, 1], [0, 1]]), (1, [[0, 1], [1, 2]]), (2, [[0, 1], [2, 3]])]:
        a, b = gather(v, p, stride)
        assert a.shape == b.shape == (outputs * width, terms, n)
        for j in range(outputs):
            for c in range(width):
                for i in range(terms):
                    assert a[j * width + c, i].tolist() == v[rows[j][i], c].tolist(), (stride, j, c, i)
                    assert b[j * width + c, i].tolist() == p[j, i].tolist()


def test_schoolbook_fold_by_hand():
    """One output, two terms, width 2, n = 2, q = 97: z_c = p_0 v_{0,c} + p_1 v_{1,c} with p_0 = 1, p_1 = X."""
    v = np.array([[[1, 2], [3, 4]], [[5, 6], [7, 8]]], dtype=np.uint64)
    p = np.array([[[1, 0], [0, 1]]], dtype=np.uint64)
    # X (5 + 6X) = -6 + 5X;  X (7 + 8X) = -8 + 7X  (mod X^2 + 1)
    assert schoolbook_fold(v, p, 0, 97, -1) == [[[(1 - 6) % 97, 7], [(3 - 8) % 97, 11]]]
    assert schoolbook_fold(v, p, 0, 97, 1) == [[[7, 7], [11, 11]]]
