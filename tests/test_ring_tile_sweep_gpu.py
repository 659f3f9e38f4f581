"""GPU suite: every arithmetic flavour and every tile log-size LT = 1 .. 12 of the fused ring tile kernels — ring_mul, ring_dot,
RingMatrix.matvec and RingMatrix.matvec_gadget.  Each LT is its own instantiation (1, 2 or 3 rounds, a last round of LT % 4 bits with
its own lane mapping, 4096/n vectors per tile), so each is launched here, in six flavours: FP64, u64 at a 60-bit and (forced) at a
44-bit prime, cyclic Goldilocks, and cyclic contexts over both ordinary primes.

Every word is compared exactly with the references of tests/ring_tile_model.py: the oracle's transforms around a pointwise product and,
at the first and last vector of the full and of the ragged tile, the schoolbook product on Python integers, which shares nothing with
any transform.  No kernel result is compared with another kernel's.

Shapes per case: batch = 4096/n + 3 (one full tile and a ragged one of three vectors; 2 at n = 4096), rows = row_block + 1 (a full and
a partial row block, with row row_block a copy of row 0), cols = 3.

Two combinations do not exist and are asserted as refusals: the gadget product on Goldilocks (no admissible (b, D)), and b = 11 under
the 60-bit prime (5 digits are 55 bits, 6 are 66 > 64), where b = 16 at its minimum D = 4 takes the place of the first pair."""
import numpy as np
import pytest

import ring_gadget_model as gadget
import ring_tile_model as model
from ring_tile_model import (FLAVOURS, GOLDILOCKS, test_planted_words_and_the_lazy_carry_element,  # noqa: F401 (collected here: CPU tests)
                             test_schoolbook_by_hand, test_schoolbook_equals_oracle_composition)

SENTINEL = 0x5A5A5A5A5A5A5A5A
F64_FLAVOURS = ("f64", "cyc_f64")


def _open(pkg, lib, flavour, n, omega):
    q, cyclic = FLAVOURS[flavour]
    lib.lsr_set_arith_mode(1 if flavour == "u64_q44" else 0)
    try:
        if not cyclic:
            ctx = pkg.NttContext(q, n, device=0)
        elif q == GOLDILOCKS:
            ctx = pkg.CyclicNtt(n)
        else:
            ctx = pkg.CyclicNtt(n, modulus=q, omega=omega)
    finally:
        lib.lsr_set_arith_mode(0)
    assert bool(lib.lsr_ntt_context_uses_f64(ctx.handle)) == (flavour in F64_FLAVOURS), flavour
    assert lib.lsr_ntt_context_is_cyclic(ctx.handle) == int(cyclic), flavour
    assert not cyclic or ctx.omega == omega
    return q, cyclic, ctx


def _row_block(ctx, n):
    probe = ctx.ring_matrix(np.zeros((1, 1, n), dtype=np.uint64))
    block = probe.row_block
    probe.close()
    return block


def _dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _guarded(torch, batch, rows, n):
    """A device output of batch + 1 vectors filled with a sentinel: the last one lies behind the ragged tile and must stay as it is."""
    return torch.full((batch + 1, rows, n), SENTINEL, dtype=torch.int64, device="cuda")


def _check_guarded(d_y, want, what):
    got = _host(d_y)
    assert np.array_equal(got[:-1], want), what
    assert bool((got[-1] == np.uint64(SENTINEL)).all()), (what, "the vector behind the batch was written")


def _edge_vectors(logn, per_tile, batch):
    """The vectors also held against the schoolbook: first and last of the full tile and of the ragged tile (n <= 64), the last one
    (n = 128, 256), none above: the O(n^2) product in Python bounds the test's time."""
    if logn <= 6:
        return sorted({0, per_tile - 1, per_tile, batch - 1})
    return [batch - 1] if logn <= 8 else []


@pytest.mark.gpu
@pytest.mark.parametrize("logn", range(1, 13))
@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_every_flavour_and_tile_size(pkg, lib, oracle, flavour, logn):
    import torch
    n = 1 << logn
    omega = model.omega_for(oracle, flavour, n)
    q, cyclic, ctx = _open(pkg, lib, flavour, n, omega)
    sign = 1 if cyclic else -1
    per_tile = 4096 >> logn
    batch = per_tile + 3 if logn < 12 else 2
    block = _row_block(ctx, n)
    rows, cols, terms = block + 1, 3, 3
    edges = _edge_vectors(logn, per_tile, batch)
    rng = np.random.default_rng(100 * logn + len(flavour))
    ref = lambda fn, *args: fn(oracle, q, n, *args, cyclic, omega)      # noqa: E731
    lazy = model.goldilocks_lazy_carry(n) if flavour == "gold" and n >= 4 else None
    where = (flavour, n)

    # 1. ring_mul: per-product b, one shared b
    a, b = model.planted(rng, q, batch, n), model.planted(rng, q, batch, n)
    if lazy is not None:
        a[1] = b[1] = lazy
    got_each, got_shared = ctx.ring_mul(a, b), ctx.ring_mul(a, b[batch - 1])
    assert np.array_equal(got_each, ref(model.oracle_product, a, b)), (where, "ring_mul")
    assert np.array_equal(got_shared, ref(model.oracle_product, a, b[batch - 1])), (where, "ring_mul, shared b")
    for j in edges:
        assert got_each[j].tolist() == model.schoolbook(a[j], b[j], q, sign), (where, "ring_mul", j)
        assert got_shared[j].tolist() == model.schoolbook(a[j], b[batch - 1], q, sign), (where, "ring_mul, shared b", j)

    # 2. ring_dot: per-output b, one shared b
    a, b = model.planted(rng, q, batch * terms, n).reshape(batch, terms, n), model.planted(rng, q, batch * terms, n).reshape(batch, terms, n)
    if lazy is not None:
        a[1, 0] = b[1, 2] = b[batch - 1, 1] = lazy
    got_each, got_shared = ctx.ring_dot(a, b), ctx.ring_dot(a, b[batch - 1])
    assert np.array_equal(got_each, ref(model.oracle_dot, a, b)), (where, "ring_dot")
    assert np.array_equal(got_shared, ref(model.oracle_dot, a, b[batch - 1])), (where, "ring_dot, shared b")
    if edges:
        assert got_each[edges].tolist() == model.schoolbook_dot(a[edges], b[edges], q, sign), (where, "ring_dot", edges)
        assert got_shared[edges].tolist() == model.schoolbook_dot(a[edges], b[batch - 1], q, sign), (where, "ring_dot, shared b", edges)

    # 3. ring_matvec: the host form (M copied, then transformed) and the device forms (M transformed from the caller's device buffer)
    def matrix(columns):
        m = model.planted(rng, q, rows * columns, n).reshape(rows, columns, n)
        m[1] = q - 1
        m[block] = m[0]              # the partial row block must return the full block's words
        return m

    def check_rows(got, m, x, what):
        """got [batch, rows, n] of M x: the oracle's composition everywhere, the schoolbook at the edge vectors (the copy of row 0 is
        held against row 0's product)."""
        assert np.array_equal(got, ref(model.oracle_matvec, m, x)), (where, what)
        assert np.array_equal(got[:, block], got[:, 0]), (where, what, "partial row block")
        if edges:
            assert got[edges][:, :block].tolist() == model.schoolbook_matvec(m[:block], x[edges], q, sign), (where, what, edges)

    m, x = matrix(cols), model.planted(rng, q, batch * cols, n).reshape(batch, cols, n)
    if lazy is not None:
        x[1, 0] = m[0, 1] = m[block, 1] = lazy
    mat = ctx.ring_matrix(m)
    got = mat.matvec(x)
    check_rows(got, m, x, "matvec")
    mat.close()
    d_m, d_x, d_y = _dev(torch, m), _dev(torch, x), _guarded(torch, batch, rows, n)
    dev_mat = ctx.ring_matrix_device(d_m.data_ptr(), rows, cols, _stream(torch))
    dev_mat.matvec_device(d_y.data_ptr(), d_x.data_ptr(), batch, _stream(torch))
    torch.cuda.synchronize()
    _check_guarded(d_y, got, (where, "matvec_device on ring_matrix_device"))
    dev_mat.close()

    # 4. matvec_gadget against the oracle's mat-vec of the model's digits
    if flavour == "gold":
        mat = ctx.ring_matrix(np.zeros((1, 2, n), dtype=np.uint64))
        for base_log2, digits in [(32, 2), (11, 2), (4, 2)]:
            assert not gadget.admissible(q, base_log2, digits)
            with pytest.raises(pkg.CoreError, match="not admissible"):
                mat.matvec_gadget(np.zeros((1, 1, n), dtype=np.uint64), base_log2, digits)
        mat.close()
        ctx.close()
        return
    pairs = model.gadget_pairs(q)
    if pairs[0][0] != 11:            # the 60-bit prime: no digit count is admissible at b = 11
        assert gadget.min_digits(q, 11) == 0 and pkg.ring_gadget_min_digits(q, 11) == 0
        mat = ctx.ring_matrix(np.zeros((1, 5, n), dtype=np.uint64))
        with pytest.raises(pkg.CoreError, match="not admissible"):
            mat.matvec_gadget(np.zeros((1, 1, n), dtype=np.uint64), 11, 5)
        mat.close()
    for base_log2, digits, xcols in pairs:
        what = "matvec_gadget b = %d, D = %d" % (base_log2, digits)
        assert digits == pkg.ring_gadget_min_digits(q, base_log2)
        m, x = matrix(xcols * digits), model.planted(rng, q, batch * xcols, n).reshape(batch, xcols, n)
        z = gadget.gadget_inverse(x, q, base_log2, digits)
        mat = ctx.ring_matrix(m)
        got = mat.matvec_gadget(x, base_log2, digits)
        check_rows(got, m, z, what)
        mat.close()
        d_m, d_x, d_y = _dev(torch, m), _dev(torch, x), _guarded(torch, batch, rows, n)
        dev_mat = ctx.ring_matrix_device(d_m.data_ptr(), rows, xcols * digits, _stream(torch))
        dev_mat.matvec_gadget_device(d_y.data_ptr(), d_x.data_ptr(), batch, base_log2, digits, _stream(torch))
        torch.cuda.synchronize()
        _check_guarded(d_y, got, (where, what, "device form"))
        dev_mat.close()
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("logn", [5, 10, 11])
@pytest.mark.parametrize("flavour", F64_FLAVOURS)
def test_f64_accumulators_at_partial_round_sizes(pkg, lib, oracle, flavour, logn):
    """Last rounds of 1, 2 and 3 bits behind full rounds.  33 identical columns: each of a full row block's accumulators receives the
    same product 33 times, every one of one sign per residue, across the re-centring after column 31; y = 33 (m0 x0).  Then the gadget
    kernel over 36 columns (b = 4, D = 12, xcols = 3) with every entry of M all q - 1."""
    n = 1 << logn
    omega = model.omega_for(oracle, flavour, n)
    q, cyclic, ctx = _open(pkg, lib, flavour, n, omega)
    assert pkg.RING_DOT_F64_RECENTRE_PERIOD == 32
    rng = np.random.default_rng(logn + len(flavour))
    rows, cols = _row_block(ctx, n), 33
    m0, x0 = model.planted(rng, q, 1, n), model.planted(rng, q, 1, n)
    one = model.oracle_product(oracle, q, n, m0, x0, cyclic, omega)[0]
    want = np.array([int(v) * cols % q for v in one], dtype=np.uint64)
    mat = ctx.ring_matrix(np.ascontiguousarray(np.broadcast_to(m0[0], (rows, cols, n))))
    got = mat.matvec(np.ascontiguousarray(np.broadcast_to(x0[0], (1, cols, n))))
    assert got.shape == (1, rows, n)
    for r in range(rows):
        assert np.array_equal(got[0, r], want), (flavour, n, r)
    mat.close()

    base_log2, digits, xcols = 4, 12, 3
    assert gadget.min_digits(q, base_log2) == digits and xcols * digits > pkg.RING_DOT_F64_RECENTRE_PERIOD
    m = np.full((rows, xcols * digits, n), q - 1, dtype=np.uint64)
    x = model.planted(rng, q, xcols, n).reshape(1, xcols, n)
    want = model.oracle_matvec(oracle, q, n, m, gadget.gadget_inverse(x, q, base_log2, digits), cyclic, omega)
    mat = ctx.ring_matrix(m)
    assert np.array_equal(mat.matvec_gadget(x, base_log2, digits), want), (flavour, n, "gadget")
    mat.close()
    ctx.close()
