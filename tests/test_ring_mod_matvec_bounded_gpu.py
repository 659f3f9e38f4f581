"""GPU suite: the bounded resident-matrix product under an arbitrary modulus (RingModMatrix.matvec_bounded / matvec_bounded_device,
lsr_ring_mod_matvec_bounded_batch, batch.h "resident matrices under any modulus").  Every output word and every status
is compared exactly: with the Python-integer model (tests/ring_mod_matvec_bounded_model.py: no primes, no groups) or — where the
model would take more than seconds — with the plain product, the handle's inner product or its multiply, which the contract names
as the definition.  Device outputs are one vector longer than the call needs and come back with that tail untouched; y and status
are pre-filled with sentinels.

What the shapes are for: a tile of the kernel spans several vectors (2048 at n = 2, 64 at n = 64, 2 at n = 2048), so a violation has
to reach the flag word of ITS vector and no other; a ragged last tile clips lanes whose vectors are absent; a later column group
finds its violation after the earlier groups were reduced into y."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import ring_mod_matvec_bounded_model as model
import ring_mod_model as mod

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P5 = mod.prime_5_mod_8_below(1 << 32)
Q40 = model.Q40
SENTINEL = 0x5A5A5A5A5A5A5A5A
STATUS_SENTINEL = 7
SUM_WORDS = 1 << 22                        # the handle's workspace per prime
FLAG_WORDS = 4096                          # the handle's per-vector flag words: the most vectors of one chunk (batch.h)
ROWS, COLS = 5, 3                          # rows 5: more than one row block in both flavours (4 and 2)


def _dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.uint64)).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _random(rng, q, shape):
    return rng.integers(0, q, size=shape, dtype=np.uint64)


def _short(rng, q, shape, bound):
    return (rng.integers(-bound, bound + 1, size=shape) % q).astype(np.uint64)


def _bounded_device(torch, mat, x, bound=0):
    """matvec_bounded_device on a numpy x [batch][cols][n] -> (y [batch][rows][n], status [batch]), the guards checked"""
    batch = x.shape[0]
    d_x = _dev(torch, x)
    d_y = torch.full((batch + 1, mat.rows, mat.n), SENTINEL, dtype=torch.int64, device="cuda")
    d_status = torch.full((batch + 1,), STATUS_SENTINEL, dtype=torch.int32, device="cuda")
    mat.matvec_bounded_device(d_y.data_ptr(), d_status.data_ptr(), d_x.data_ptr(), batch, bound, stream=_stream(torch))
    torch.cuda.synchronize()
    y, status = _host(d_y), d_status.cpu().numpy()
    assert bool((y[-1] == np.uint64(SENTINEL)).all()) and status[-1] == STATUS_SENTINEL, "the words behind y or status were written"
    return y[:-1], status[:-1]


def _plain_device(torch, mat, x):
    d_x = _dev(torch, x)
    d_y = torch.full((x.shape[0], mat.rows, mat.n), -1, dtype=torch.int64, device="cuda")
    mat.matvec_device(d_y.data_ptr(), d_x.data_ptr(), x.shape[0], stream=_stream(torch))
    torch.cuda.synchronize()
    return _host(d_y)


def _gated(plain, status):
    """the plain product with the vectors of a status other than 1 zeroed"""
    want = plain.copy()
    want[np.asarray(status) != 1] = 0
    return want


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- 1. clean inputs ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _clean_reference(n, q):
    """operands and the model's product, computed once and read-only: x with the centred extremes in whole polynomials, and xs drawn
    within min(floor(q/2), 100)"""
    rng = np.random.default_rng(3800 + 7 * n + q % 991)
    short = min(q // 2, 100)
    m, x, xs = _random(rng, q, (ROWS, COLS, n)), _random(rng, q, (3, COLS, n)), _short(rng, q, (3, COLS, n), short)
    x[0, 0, :], x[1, 0, :] = q // 2, min(q // 2 + 1, q - 1)
    xs[0, 0, :], xs[2, COLS - 1, :] = short, q - short
    want, want_s = model.matvec_bounded(m, x, q), model.matvec_bounded(m, xs, q, short)
    for a in (m, x, xs) + want + want_s:
        a.setflags(write=False)
    return m, x, xs, short, want, want_s


@pytest.mark.parametrize("n,q", [(2, 2), (4, 3329), (64, P5), (256, 3329), (64, 1 << 32)])
def test_clean_inputs_equal_the_model_and_the_plain_product(pkg, n, q):
    import torch
    m, x, xs, short, want, want_s = _clean_reference(n, q)
    assert want[1].tolist() == [1, 1, 1] == want_s[1].tolist()
    with pkg.RingMod(q, n, device=0) as ring, ring.matrix(m) as mat:
        plain, plain_s = _plain_device(torch, mat, x), _plain_device(torch, mat, xs)
        assert np.array_equal(plain, want[0]) and np.array_equal(plain_s, want_s[0])
        for bound in (0, q // 2):
            assert _same(_bounded_device(torch, mat, x, bound), want), (n, q, bound)
            assert _same(_bounded_device(torch, mat, xs, bound), want_s), (n, q, bound)
        assert _same(_bounded_device(torch, mat, xs, short), want_s), (n, q, short)
        assert _same(mat.matvec_bounded(xs, short), want_s), "host"
        assert _same(mat.matvec_bounded(x), want), "host, no bound"
        y, status = mat.matvec_bounded(xs[1], short)                   # a 2-d x: one vector
        assert status == 1 and np.array_equal(y, want_s[0][1])


# ---- 2. a violation stays with its vector --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,q,batch,planted", [
    (64, P5, 67, {5: "over", 6: "high", 65: "over", 66: "both"}),         # one full tile of 64 vectors and a ragged one of 3
    (2, P5, 2051, {5: "over", 6: "high", 2049: "over", 2050: "both"}),    # 2048 vectors in the full tile
    (2048, P5, 3, {1: "both"}),                                           # 2 vectors per tile, the ragged tile holds one
    (4096, 1 << 32, 2, {0: "over"}),                                      # one vector per tile
])
def test_a_violation_stays_with_its_vector(pkg, n, q, batch, planted):
    """the violations sit in the last word of the last column (`both`: over the bound in the word before it, >= q in the last)"""
    import torch
    bound = 1000
    rng = np.random.default_rng(n + batch)
    m, clean = _random(rng, q, (ROWS, COLS, n)), _short(rng, q, (batch, COLS, n), bound)
    x, status = clean.copy(), [1] * batch
    for j, kind in planted.items():
        if kind == "over":
            x[j, COLS - 1, n - 1] = bound + 1
        else:
            x[j, COLS - 1, n - 1] = q
        if kind == "both":
            x[j, COLS - 1, n - 2] = q - bound - 1
        status[j] = 0 if kind == "over" else -1
    with pkg.RingMod(q, n, device=0) as ring, ring.matrix(m) as mat:
        plain = _plain_device(torch, mat, clean)
        if n <= 64:
            assert np.array_equal(plain[:8], model.matvec_bounded(m, clean[:8], q, bound)[0])
        y, got = _bounded_device(torch, mat, x, bound)
        assert got.tolist() == status
        assert np.array_equal(y, _gated(plain, status))
        for j in planted:
            assert not y[j].any() and all(y[i].any() for i in (j - 1, j + 1) if 0 <= i < batch and i not in planted)
        assert _same(_bounded_device(torch, mat, clean, bound), (plain, np.ones(batch, dtype=np.int32)))


# ---- 3. the exact boundary -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,q,bound", [(64, 3329, 5), (64, P5, 1 << 20), (256, Q40 - 16, 0)])
def test_the_bound_is_inclusive_and_q_is_not(pkg, n, q, bound):
    import torch
    b = bound or q // 2
    rng = np.random.default_rng(n + bound % 97)
    m, x = _random(rng, q, (ROWS, COLS, n)), _short(rng, q, (8, COLS, n), b)
    x[0, 0, 0], x[0, COLS - 1, n - 1] = b, q - b                       # met exactly, from both sides
    status = [1, 0, 0, -1, -1, -1, -1, 1]
    x[1, 1, 3], x[2, 2, n - 1] = b + 1, q - b - 1                      # missed by one
    x[3, 0, 0], x[4, 1, 1], x[5, COLS - 1, n - 1] = q, 1 << 63, 2**64 - 1
    x[6, 0, 1], x[6, 0, 2] = b + 1, q + 1                              # -1 wins over 0
    if not bound:                                                      # every word below q is within floor(q/2): only -1 can occur
        assert q % 2 == 1 and b + 1 == q - b
        status[1] = status[2] = 1
    want = model.matvec_bounded(m, x, q, bound)
    assert want[1].tolist() == status
    with pkg.RingMod(q, n, device=0) as ring, ring.matrix(m) as mat:
        assert _same(_bounded_device(torch, mat, x, bound), want)
        assert _same(mat.matvec_bounded(x, bound), want), "host"


# ---- 4. groups -------------------------------------------------------------------------------------------------------------------------
def test_groups_follow_the_bound_and_a_late_violation_zeroes_the_vector(pkg):
    """q = 2^40 + 15, n = 64, 50 columns within floor(floor(q/2) / 3): groups of 23, 23 and 4; column 49 is read by the last alone"""
    import torch
    q, n, cols, batch = Q40, 64, 50, 3
    bound = q // 2 // 3
    assert model.groups(q, n, cols, bound) == [23, 23, 4] and len(model.groups(q, n, cols)) == 8
    assert pkg.ring_mod_capacity_bounded(q, n, bound) == 23 and pkg.ring_mod_capacity(q, n) == 7
    rng = np.random.default_rng(40)
    m, x = _random(rng, q, (ROWS, cols, n)), _short(rng, q, (batch, cols, n), bound)
    x[0, 0, :], x[2, 22, :], x[2, 49, :] = bound, q - bound, bound     # whole polynomials at the bound
    want = model.matvec_bounded(m, x, q, bound)
    assert want[1].tolist() == [1, 1, 1]
    with pkg.RingMod(q, n, device=0) as ring, ring.matrix(m) as mat:
        assert _same(_bounded_device(torch, mat, x, bound), want), "23 + 23 + 4"
        assert _same(_bounded_device(torch, mat, x, 0), want), "8 groups"
        assert np.array_equal(_plain_device(torch, mat, x), want[0])
        bad = x.copy()
        bad[1, 49, 17] = bound + 1
        want_bad = model.matvec_bounded(m, bad, q, bound)
        assert want_bad[1].tolist() == [1, 0, 1] and not want_bad[0][1].any() and np.array_equal(want_bad[0][[0, 2]], want[0][[0, 2]])
        assert _same(_bounded_device(torch, mat, bad, bound), want_bad)
        bad[1, 49, 17] = q                                              # the same under no bound: the eighth group finds it
        got = _bounded_device(torch, mat, bad, 0)
        assert got[1].tolist() == [1, -1, 1] and np.array_equal(got[0], _gated(want[0], [1, -1, 1]))


# ---- 5. a chunk boundary ---------------------------------------------------------------------------------------------------------------
def test_one_vector_past_a_chunk(pkg):
    """n = 64, rows 5: the sums hold 13107 vectors, the flag words 4096 — the smaller caps the chunk.  Violations in the last vector of
    the first chunk and in the only vector of the second; the reference is the handle's inner product, row by row"""
    import torch
    n, q, rows, cols = 64, P5, 5, 2
    batch = min(SUM_WORDS // (rows * n), FLAG_WORDS) + 1
    assert batch == FLAG_WORDS + 1
    rng = np.random.default_rng(66)
    m, x = _random(rng, q, (rows, cols, n)), _random(rng, q, (batch, cols, n))
    clean = x.copy()
    x[batch - 2, 1, n - 1], x[batch - 1, 0, 0] = q, 1 << 63
    d_x, d_clean = _dev(torch, x), _dev(torch, clean)
    d_y = torch.full((batch + 1, rows, n), SENTINEL, dtype=torch.int64, device="cuda")
    d_status = torch.full((batch + 1,), STATUS_SENTINEL, dtype=torch.int32, device="cuda")
    d_c = torch.empty((batch, n), dtype=torch.int64, device="cuda")
    with pkg.RingMod(q, n, device=0) as ring, ring.matrix(m) as mat:
        mat.matvec_bounded_device(d_y.data_ptr(), d_status.data_ptr(), d_x.data_ptr(), batch, 0, stream=_stream(torch))
        for r in range(rows):
            d_b = _dev(torch, m[r])
            ring.dot_device(d_c.data_ptr(), d_clean.data_ptr(), d_b.data_ptr(), batch, cols, 1, stream=_stream(torch))
            assert torch.equal(d_y[:batch - 2, r], d_c[:batch - 2]), r
        torch.cuda.synchronize()
        assert d_status.cpu().tolist() == [1] * (batch - 2) + [-1, -1, STATUS_SENTINEL]
        assert not bool(d_y[batch - 2:batch].any()) and bool((d_y[batch] == SENTINEL).all())


# ---- 6. row ranges ---------------------------------------------------------------------------------------------------------------------
def test_a_flagged_vector_is_zero_in_every_row_range(pkg):
    """rows n above the workspace: one vector and 1024 rows at a time, then the last row.  The word >= q sits at the end of x[0]: the
    first range's reduce must know of it already"""
    import torch
    n, q, rows, batch = 4096, 1 << 32, SUM_WORDS // 4096 + 1, 2
    rng = np.random.default_rng(1025)
    d_m = _dev(torch, _random(rng, q, (rows, 1, n)))
    x = _random(rng, q, (batch, 1, n))
    x[0, 0, n - 1] = q
    d_x = _dev(torch, x)
    d_y = torch.full((batch + 1, rows, n), SENTINEL, dtype=torch.int64, device="cuda")
    d_status = torch.full((batch + 1,), STATUS_SENTINEL, dtype=torch.int32, device="cuda")
    d_c = torch.empty((rows, n), dtype=torch.int64, device="cuda")
    with pkg.RingMod(q, n, device=0) as ring, ring.matrix_device(d_m.data_ptr(), rows, 1, stream=_stream(torch)) as mat:
        mat.matvec_bounded_device(d_y.data_ptr(), d_status.data_ptr(), d_x.data_ptr(), batch, 0, stream=_stream(torch))
        ring.mul_device(d_c.data_ptr(), d_m.data_ptr(), d_x[1].data_ptr(), rows, 1, stream=_stream(torch))
        torch.cuda.synchronize()
        assert d_status.cpu().tolist() == [-1, 1, STATUS_SENTINEL]
        assert not bool(d_y[0].any()), "every row range of the flagged vector"
        assert torch.equal(d_y[1], d_c) and bool((d_y[2] == SENTINEL).all())


# ---- 7. all twelve tile sizes, both flavours -------------------------------------------------------------------------------------------
def _sweep_shape(logn):
    """(batch, the violating vector of the full tile, the one of the ragged tile): 4096 / n vectors fill a tile and 3 more make a
    ragged one (n = 4096: two tiles of one vector).  The index within the full tile alternates between 0x555 and 0xAAA cut to the
    tile, so that over the twelve sizes every one of its eleven low bits is set at some size and clear at another"""
    per_tile = 4096 >> logn
    if per_tile == 1:
        return 2, 0, 1
    return per_tile + 3, (0x555 if logn & 1 else 0xAAA) & (per_tile - 1), per_tile + logn % 3


@functools.lru_cache(maxsize=None)
def _sweep_operands(logn):
    n = 1 << logn
    q = min(mod.largest_admissible(n), P5)
    batch = _sweep_shape(logn)[0]
    rng = np.random.default_rng(3800 + logn)
    m, x = _random(rng, q, (3, 2, n)), _short(rng, q, (batch, 2, n), 1000)
    m.setflags(write=False)
    x.setflags(write=False)
    return q, m, x


@pytest.mark.parametrize("logn", range(1, 13))
def test_every_tile_size_and_both_flavours(pkg, lib, logn):
    """rows 3, cols 2; one violating vector per run — in the full tile, then in the ragged one — over the bound at odd log n, >= q
    at even; both flavours against the plain product of the FP64 handle on the clean vectors"""
    import torch
    n, bound = 1 << logn, 1000
    q, m, clean = _sweep_operands(logn)
    batch, in_full, in_ragged = _sweep_shape(logn)
    assert q == P5 and mod.capacity(q, n) >= 1
    lib.lsr_set_arith_mode(1)
    try:
        integer = pkg.RingMod(q, n, device=0)
    finally:
        lib.lsr_set_arith_mode(0)
    with integer, pkg.RingMod(q, n, device=0) as fp64:
        assert not integer.prime_context(0).uses_f64 and fp64.prime_context(0).uses_f64
        with integer.matrix(m) as mi, fp64.matrix(m) as mf:
            plain = _plain_device(torch, mf, clean)
            if logn <= 6:
                assert np.array_equal(plain[:2], model.matvec_bounded(m, clean[:2], q, bound)[0])
            for name, mat in (("integer", mi), ("fp64", mf)):
                assert _same(_bounded_device(torch, mat, clean, bound), (plain, np.ones(batch, dtype=np.int32))), (name, "clean")
                for j in (in_full, in_ragged):
                    x, status = clean.copy(), [1] * batch
                    x[j, 1, n - 1], status[j] = (bound + 1, 0) if logn & 1 else (q, -1)
                    y, got = _bounded_device(torch, mat, x, bound)
                    assert got.tolist() == status, (name, j, np.nonzero(got != 1)[0].tolist())
                    assert np.array_equal(y, _gated(plain, status)), (name, j)


# ---- 7b. operands and outputs off the vector alignment ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 512])
@pytest.mark.parametrize("flavour", ["f64", "u64"])
def test_operands_and_outputs_off_the_vector_alignment(pkg, lib, flavour, n):
    """x and y start one word into their allocations: 8-byte but not 16-byte aligned, where the host takes the one-word-per-lane
    variants of the check pass and of the reduces (the tile kernels read x where it lies).  q is the largest admissible modulus at
    this n: within floor(q/2) / 2 two columns are a group, so three columns are a plain and an accumulating gated reduce — behind a
    check pass of its own at n = 64, with the check in the tile at n = 512.  Vector 1 holds a word one over the bound and vector 2 a
    word >= q, both in the last column, which the second group alone reads: they come back as zeros by the one-word zero-fill.  The
    plain product of the same matrix takes its columns one at a time (three reduces, two accumulating), the gadget product in one
    group.  The word before y, the word behind it and the words behind status stay as they were, and so does x."""
    import torch
    import ring_mod_matvec_model as plain_model
    rows, cols, batch, base_log2, digits = 3, 3, 4, 14, 3
    q = mod.largest_admissible(n)
    bound = q // 2 // 2
    assert model.groups(q, n, cols, bound) == [2, 1] and model.groups(q, n, cols) == [1, 1, 1] == [mod.capacity(q, n)] * cols
    assert plain_model.capacity_bounded(q, n, 1 << (base_log2 - 1)) >= cols
    rng = np.random.default_rng(817 + n)
    lib.lsr_set_arith_mode(0 if flavour == "f64" else 1)
    try:
        ring = pkg.RingMod(q, n, device=0)
    finally:
        lib.lsr_set_arith_mode(0)

    def run(call, x, with_status):
        d_x = torch.full((x.size + 2,), SENTINEL, dtype=torch.int64, device="cuda")
        d_x[1:1 + x.size].copy_(_dev(torch, x).reshape(-1))
        words = batch * rows * n
        d_y = torch.full((words + 3,), SENTINEL, dtype=torch.int64, device="cuda")
        d_status = torch.full((batch + 2,), STATUS_SENTINEL, dtype=torch.int32, device="cuda")
        assert (d_x.data_ptr() + 8) % 16 == 8 and (d_y.data_ptr() + 8) % 16 == 8
        call(d_y.data_ptr() + 8, d_status.data_ptr(), d_x.data_ptr() + 8)
        torch.cuda.synchronize()
        y, status = _host(d_y), d_status.cpu().numpy()
        assert y[0] == SENTINEL and (y[1 + words:] == SENTINEL).all(), "the words around y were written"
        assert status[batch if with_status else 0:].tolist() == [STATUS_SENTINEL] * (2 if with_status else batch + 2), "status was written past the call's"
        assert np.array_equal(_host(d_x)[1:-1], x.reshape(-1)) and _host(d_x)[0] == SENTINEL == _host(d_x)[-1], "x was written"
        return y[1:1 + words].reshape(batch, rows, n), status[:batch]

    with ring:
        assert ring.prime_context(0).uses_f64 == (flavour == "f64") == ring.prime_context(1).uses_f64
        m = _random(rng, q, (rows, cols, n))
        with ring.matrix(m) as mat:
            s = _stream(torch)
            x = _short(rng, q, (batch, cols, n), bound)
            x[0, 0, :], x[3, cols - 1, :] = bound, q - bound                                  # whole polynomials at the bound
            want = model.matvec_bounded(m, x, q, bound)
            assert want[1].tolist() == [1] * batch and all(want[0][j].any() for j in range(batch))
            assert _same(run(lambda y, st, dx: mat.matvec_bounded_device(y, st, dx, batch, bound, stream=s), x, True), want)
            bad = x.copy()
            bad[1, cols - 1, n - 1], bad[2, cols - 1, n - 1] = bound + 1, q
            want = model.matvec_bounded(m, bad, q, bound)
            got = run(lambda y, st, dx: mat.matvec_bounded_device(y, st, dx, batch, bound, stream=s), bad, True)
            assert want[1].tolist() == [1, 0, -1, 1] and _same(got, want)
            assert not got[0][1:3].any() and got[0][0].any() and got[0][3].any()
            # no bound stated: three groups of one column, and only -1 can occur
            want = model.matvec_bounded(m, bad, q)
            got = run(lambda y, st, dx: mat.matvec_bounded_device(y, st, dx, batch, 0, stream=s), bad, True)
            assert want[1].tolist() == [1, 1, -1, 1] and _same(got, want) and not got[0][2].any()
            # the plain and the gadget product of the same matrix
            full = _random(rng, q, (batch, cols, n))
            full[0, 0, :], full[1, 0, :] = q // 2, q // 2 + 1
            got = run(lambda y, st, dx: mat.matvec_device(y, dx, batch, stream=s), full, False)
            assert np.array_equal(got[0], plain_model.matvec(m, full, q))
            narrow = _random(rng, q, (batch, cols // digits, n))
            narrow[0, 0, :3] = [q // 2, q // 2 + 1, q - 1]
            got = run(lambda y, st, dx: mat.matvec_gadget_device(y, dx, batch, base_log2, digits, stream=s), narrow, False)
            assert np.array_equal(got[0], plain_model.matvec_gadget(m, narrow, q, base_log2, digits))


# ---- 8. capture ------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_straight_after_create(pkg):
    """no eager bounded call first: the flag words exist since the handle's create.  Three groups inside the graph; two replays on
    fresh x, the second with a violation that only the last group reads"""
    import torch
    q, n, cols, batch = Q40, 64, 50, 5
    bound = q // 2 // 3
    rng = np.random.default_rng(99)
    m = _random(rng, q, (ROWS, cols, n))
    ring, eager_ring = pkg.RingMod(q, n, device=0), pkg.RingMod(q, n, device=0)
    mat = ring.matrix_device(_dev(torch, m).data_ptr(), ROWS, cols, stream=_stream(torch))
    eager = eager_ring.matrix(m)
    d_x = torch.zeros((batch, cols, n), dtype=torch.int64, device="cuda")
    d_y = torch.full((batch, ROWS, n), SENTINEL, dtype=torch.int64, device="cuda")
    d_status = torch.full((batch,), STATUS_SENTINEL, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        mat.matvec_bounded_device(d_y.data_ptr(), d_status.data_ptr(), d_x.data_ptr(), batch, bound, stream=torch.cuda.current_stream().cuda_stream)
    for replay in range(2):
        x = _short(rng, q, (batch, cols, n), bound)
        if replay == 1:
            x[3, 49, n - 1] = bound + 1                                 # the flags are cleared and set anew inside the graph
        d_x.copy_(_dev(torch, x))
        graph.replay()
        torch.cuda.synchronize()
        got = (_host(d_y).copy(), d_status.cpu().numpy())
        assert got[1].tolist() == ([1] * batch if replay == 0 else [1, 1, 1, 0, 1])
        assert _same(got, _bounded_device(torch, eager, x, bound)), replay
        assert bool(got[0][3].any()) == (replay == 0)
    assert _same(got, model.matvec_bounded(m, x, q, bound))
    mat.close()
    eager.close()
    ring.close()                               # free while idle
    eager_ring.close()


# ---- 9. host staging -------------------------------------------------------------------------------------------------------------------
_STAGED = dict(q=P5, n=64, rows=5, cols=3, batch=600, bound=1 << 20)


def _staged_operands():
    """n = 64, rows 5, cols 3: 513 staged words a vector — under LAMBDA_SNARK_STAGING_MIB=1 255 vectors a chunk, 600 vectors in three"""
    c = _STAGED
    rng = np.random.default_rng(90)
    m = _random(rng, c["q"], (c["rows"], c["cols"], c["n"]))
    x = _short(rng, c["q"], (c["batch"], c["cols"], c["n"]), c["bound"])
    x[10, 0, 0], x[254, 2, 63], x[255, 0, 0], x[599, 2, 63] = c["bound"] + 1, c["q"], c["bound"], c["q"] - c["bound"] - 1
    return m, x


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as entry
import test_ring_mod_matvec_bounded_gpu as t
pkg, c = entry.load_package(), t._STAGED
m, x = t._staged_operands()
with pkg.RingMod(c["q"], c["n"], device=0) as ring, ring.matrix(m) as mat:
    y, status = mat.matvec_bounded(x, c["bound"])
np.savez(sys.argv[2], y=y, status=status)
"""


def test_plain_form_over_several_staged_chunks_equals_the_device_form(pkg, tmp_path):
    import torch
    assert "LAMBDA_SNARK_STAGING_MIB" not in os.environ
    script, out = tmp_path / "child.py", tmp_path / "out.npz"
    script.write_text(_CHILD)
    subprocess.run([sys.executable, str(script), ROOT, str(out)], check=True, env=dict(os.environ, LAMBDA_SNARK_STAGING_MIB="1"), timeout=300)
    got = np.load(str(out))
    c = _STAGED
    m, x = _staged_operands()
    with pkg.RingMod(c["q"], c["n"], device=0) as ring, ring.matrix(m) as mat:
        want_y, want_status = _bounded_device(torch, mat, x, c["bound"])
    assert want_status.tolist().count(1) == 597 and want_status[10] == 0 and want_status[254] == -1 and want_status[599] == 0
    assert not want_y[599].any() and want_y[255].any() and want_y[598].any()
    assert np.array_equal(got["y"], want_y) and np.array_equal(got["status"], want_status)
