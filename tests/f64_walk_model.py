"""Model of an FP64 running sum that is NOT re-centred, pure Python/numpy: which evaluation positions of a long sum of
identical products can tell a kernel that re-centres every kRingDotF64Period products from one that does not.

A double holds every integer below 2^53, and the kernels re-centre after the last product anyway, so a lost periodic re-centre changes
an output word only where a partial sum stops being an exact integer.  With identical terms the product at a position is the same
double every time and the sum walks linearly: v, 2 v, 3 v, ...  mulmod_f64 returns SOME integer = a b (mod q) of magnitude
<= 0.875 q; which of the (at most two) such integers it returns depends on the operands' doubles, not on the residue alone, so a
position counts only when the walk is inexact under EVERY admissible representative.

The tests at the bottom need no GPU; tests/test_f64_long_sums_gpu.py re-exports them so that the suite collects them."""
from itertools import product as _combinations

import numpy as np

Q44 = 17592180539393           # the 44-bit prime of the FP64 flavours (tests/ring_gadget_model.py)
MAX_DISTINCT = 3               # distinct products per cycle: at most 2^3 combinations of representatives


def representatives(c, q):
    """The integers = c (mod q) of magnitude <= 0.875 q (mulmod_f64's bound), ascending: one or two."""
    c, q = int(c) % int(q), int(q)
    return [r for r in (c - q, c) if 8 * abs(r) <= 7 * q]


def _object_rows(values):
    """values -> (object array [cycle][positions], scalar?)"""
    rows = [np.atleast_1d(np.array(v, dtype=object)) for v in values]
    return np.stack(rows), all(np.ndim(v) == 0 for v in values)


def walk_is_inexact(values, steps, start=0):
    """True where adding the cycle values[0], values[1], ... (Python ints, each an exact double) `steps` times in sequence in float64,
    beginning at `start` (an int, or one per position), ends away from the exact integer sum.  values: a sequence of ints, or of
    equally long sequences of ints (one walk per position: returns a bool array)."""
    cycle, scalar = _object_rows(values)
    period, positions = cycle.shape
    first = np.broadcast_to(np.array(start, dtype=object), (positions,))
    as_double, acc = cycle.astype(np.float64), first.astype(np.float64)
    assert all(int(d) == int(v) for d, v in zip(as_double.ravel(), cycle.ravel())), "an addend is no exact double"
    assert all(int(d) == int(v) for d, v in zip(acc, first)), "a starting value is no exact double"
    for s in range(steps):
        acc = acc + as_double[s % period]
    whole, rest = divmod(steps, period)
    exact = [int(first[k]) + whole * sum(int(v) for v in cycle[:, k]) + sum(int(v) for v in cycle[:rest, k]) for k in range(positions)]
    inexact = np.array([int(a) != e for a, e in zip(acc.tolist(), exact)], dtype=bool)
    return bool(inexact[0]) if scalar else inexact


def discriminating_positions(residues, q, steps, start=0):
    """The positions at which the walk over `steps` additions of the cycle residues[0][k], residues[1][k], ... is inexact under every
    choice of representative.  residues: [distinct products <= 3][positions], canonical words mod q.  start: what the sum begins at
    (an int or one per position; an addend is loaded as the word it is, so it has one representative)."""
    res = np.array(np.asarray(residues).tolist(), dtype=object)
    assert res.ndim == 2 and 1 <= res.shape[0] <= MAX_DISTINCT, res.shape
    distinct, positions = res.shape
    q = int(q)
    told_apart = np.ones(positions, dtype=bool)
    for choice in _combinations((0, 1), repeat=distinct):          # 1: the negative representative c - q
        values = np.stack([res[d] - q * choice[d] for d in range(distinct)])
        admissible = np.array([all(8 * abs(int(values[d, k])) <= 7 * q for d in range(distinct)) for k in range(positions)], dtype=bool)
        told_apart &= ~admissible | walk_is_inexact(list(values), steps, start)
    return np.flatnonzero(told_apart)


# ---- the model's own tests (CPU only) --------------------------------------------------------------------------------------------------
def test_representatives_are_one_or_two():
    q = 97
    assert representatives(0, q) == [0] and representatives(5, q) == [5] and representatives(96, q) == [-1]
    assert representatives(12, q) == [12] and representatives(13, q) == [-84, 13]          # 8 * 85 > 7 * 97 >= 8 * 84
    assert representatives(84, q) == [-13, 84] and representatives(85, q) == [-12]
    for c in range(q):
        reps = representatives(c, q)
        assert 1 <= len(reps) <= 2 and all((r - c) % q == 0 and 8 * abs(r) <= 7 * q for r in reps)


def test_walk_by_hand():
    """2^53 + 1 is lost: after 2^53 an odd addend cannot be added exactly.  An even addend above 2^53 is not: 2^53 + 2 is a double and
    so are its first multiples.  Two steps of 2^52 + 1 reach 2^53 + 2 exactly; the third sum, 3 * 2^52 + 3, is odd and above 2^53."""
    assert float(2**53) + 1.0 == float(2**53)
    assert walk_is_inexact([1], 1, start=2**53) and not walk_is_inexact([2], 1, start=2**53)
    assert walk_is_inexact([2**53, 1], 2) and not walk_is_inexact([2**53, 2], 2)
    assert not walk_is_inexact([2**53 + 2], 1) and not walk_is_inexact([2**53 + 2], 2) and not walk_is_inexact([2**52], 4000)
    v = 2**52 + 1
    assert not walk_is_inexact([v], 1) and not walk_is_inexact([v], 2) and walk_is_inexact([v], 3)
    assert walk_is_inexact([[v, 2**52], [v, 2**52]], 3).tolist() == [True, False]        # one walk per position, a cycle of two
    assert walk_is_inexact([[2, 2]], 1, start=[2**53 + 2, 2**54 + 4]).tolist() == [False, True]
    assert discriminating_positions([[5, 7]], 97, 3001).tolist() == []
    # q = 2^53 + 5.  The residue 2^52 + 1 is lost on its third sum as itself and walks exactly as 2^52 + 1 - q = -(2^52 + 4): one exact
    # representative is enough for the position not to count.  The residue 2^52 + 2 is lost on its fifth sum as itself
    # (5 * 2^52 + 10 is no multiple of 4 above 2^54) and as -(2^52 + 3) (5 * 2^52 + 15 is odd): the position counts.
    q = 2**53 + 5
    assert representatives(3, q) == [3] and representatives(q - 3, q) == [-3]
    odd, even = 2**52 + 1, 2**52 + 2
    assert representatives(odd, q) == [odd - q, odd] and representatives(even, q) == [even - q, even]
    assert walk_is_inexact([odd], 3) and not walk_is_inexact([odd - q], 3)
    assert walk_is_inexact([even], 5) and walk_is_inexact([even - q], 5) and not walk_is_inexact([even], 4)
    assert discriminating_positions([[odd, even, 3]], q, 3).tolist() == []
    assert discriminating_positions([[odd, even, 3]], q, 5).tolist() == [1]


def test_the_table_for_q44():
    """N sequential additions of one integer, under each of its representatives.  At the 44-bit prime no position can tell at
    N = 1025: 1025 * 0.875 q < 2^54, so a walk of an EVEN integer is exact; 512 q < 2^53, so a walk of an integer of magnitude <= q / 2
    can lose only its last sum; and the two representatives differ by the odd q, so where the smaller one is odd the other is even.
    At N = 3001 about a quarter of the positions can."""
    rng = np.random.default_rng(44)
    residues = rng.integers(0, Q44, size=(1, 4096), dtype=np.uint64)
    assert len(discriminating_positions(residues, Q44, 1025)) == 0
    mid = len(discriminating_positions(residues, Q44, 2049)) / 4096
    assert 0.05 < mid < 0.25, mid                                               # measured on the CPU: 0.13
    share = len(discriminating_positions(residues, Q44, 3001)) / 4096
    assert share > 0, share
    assert 0.15 < share < 0.45, share                                           # measured on the CPU: 0.28
