"""GPU suite: the batched ring matrix-vector product y_j = M x_j with a resident matrix (RingMatrix, lsr_ntt_ring_matvec_batch(_device)).
Pinned against schoolbook convolutions (independent of the oracle), word for word against the ring inner product row by row, against
the oracle's composition INTT(sum_c NTT(M[r][c]) . NTT(x[j][c])) at every degree 2^1 .. 2^17, across the kernel's row-block boundaries,
and at the accumulator's worst case (identical entries: every product of one sign per residue)."""
import numpy as np
import pytest

from ring_tile_model import schoolbook_matvec as _schoolbook_matvec

pytestmark = pytest.mark.gpu

Q44 = 17592180539393           # 44-bit prime, 2^18 | q - 1: every n up to 2^17 (FP64 kernels)
Q_NORTH = 17592169062401       # north_star's prime (n <= 4096)
Q60 = 1152921504606584833      # 60-bit prime (u64 Shoup kernels)
GOLD = 18446744069414584321


def _rand(rng, q, shape):
    return rng.integers(0, q, size=shape, dtype=np.uint64)


def _to_u64(values):
    return np.array([int(x) for x in np.ravel(values)], dtype=np.uint64).reshape(np.shape(values))


def _by_ring_dot(ctx, m, x):
    """Row by row through the ring inner product with the row as the shared b: [batch][rows][n]."""
    return np.stack([ctx.ring_dot(x, m[r]).reshape(x.shape[0], -1) for r in range(m.shape[0])], axis=1)


def _dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _flavour_context(pkg, lib, flavour, n):
    q = Q60 if flavour == "u64_q60" else Q44
    if flavour == "u64_q44":
        lib.lsr_set_arith_mode(1)
    try:
        ctx = pkg.NttContext(q, n, device=0)
    finally:
        lib.lsr_set_arith_mode(0)
    assert ctx.uses_f64 == (flavour == "f64")
    return q, ctx


# ---- 1. schoolbook ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [12289, Q_NORTH])
@pytest.mark.parametrize("n,shape", [(2, (1, 1)), (2, (3, 2)), (2, (5, 3)), (16, (1, 1)), (16, (3, 2)), (16, (5, 3)), (256, (3, 2))])
def test_matches_schoolbook(pkg, q, n, shape):
    rows, cols = shape
    rng = np.random.default_rng(n + 10 * rows + cols + q % 1000)
    ctx = pkg.NttContext(q, n, device=0)
    m, x = _rand(rng, q, (rows, cols, n)), _rand(rng, q, (3, cols, n))
    mat = ctx.ring_matrix(m)
    assert (mat.rows, mat.cols) == (rows, cols)
    assert mat.matvec(x).tolist() == _schoolbook_matvec(m, x, q, -1), (q, n, shape)
    assert mat.matvec(x[1]).tolist() == _schoolbook_matvec(m, x[1:2], q, -1)[0], (q, n, shape, "one vector")
    mat.close()
    ctx.close()


def test_cyclic_goldilocks_matches_plain_convolution(pkg):
    n, rows, cols = 16, 5, 3
    rng = np.random.default_rng(16)
    ntt = pkg.CyclicNtt(n)
    m, x = _rand(rng, GOLD, (rows, cols, n)), _rand(rng, GOLD, (3, cols, n))
    mat = ntt.ring_matrix(m)
    assert mat.matvec(x).tolist() == _schoolbook_matvec(m, x, GOLD, 1)
    mat.close()
    ntt.close()


# ---- 2. word for word against the ring inner product ---------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", ["f64", "u64_q60", "u64_q44"])
@pytest.mark.parametrize("n,batch", [(256, 19), (4096, 2), (8192, 2), (65536, 2)])
def test_rows_equal_the_ring_inner_product(pkg, lib, flavour, n, batch):
    """n = 256, batch 19: 16 vectors per tile, so the second tile is ragged (3 vectors)."""
    q, ctx = _flavour_context(pkg, lib, flavour, n)
    rng = np.random.default_rng(n + len(flavour))
    probe = ctx.ring_matrix(np.zeros((1, 1, n), dtype=np.uint64))
    rows, cols = probe.row_block + 1, 3
    probe.close()
    m, x = _rand(rng, q, (rows, cols, n)), _rand(rng, q, (batch, cols, n))
    mat = ctx.ring_matrix(m)
    assert np.array_equal(mat.matvec(x), _by_ring_dot(ctx, m, x)), (flavour, n)
    mat.close()
    ctx.close()


# ---- 3. the oracle's composition at every degree ---------------------------------------------------------------------------------
def _batch_for(logn):      # (test_ring_dot_gpu._batch_for)
    return {8: 7, 16: 3, 17: 2}.get(logn, 5 if logn <= 12 else 2)


def _oracle_matvec(oracle, q, n, m, x):
    """The oracle's inverse transform of sum_c mul_pointwise(forward M[r][c], forward x[j][c]); the sum of cols canonical products is
    taken in 64-bit words, which cols * q < 2^64 keeps exact."""
    rows, cols = m.shape[:2]
    assert cols * q < 2**64
    batch = x.shape[0]
    fm = np.asarray(oracle.ntt_forward(q, n, np.ascontiguousarray(m.reshape(-1, n)))).reshape(rows, cols, n)
    fx = np.asarray(oracle.ntt_forward(q, n, np.ascontiguousarray(x.reshape(-1, n)))).reshape(batch, cols, n)
    lhs = np.ascontiguousarray(np.broadcast_to(fm[None], (batch, rows, cols, n))).reshape(-1, n)
    rhs = np.ascontiguousarray(np.broadcast_to(fx[:, None], (batch, rows, cols, n))).reshape(-1, n)
    prod = np.asarray(oracle.mul_pointwise(q, n, lhs, rhs), dtype=np.uint64).reshape(batch, rows, cols, n)
    summed = np.ascontiguousarray(prod.sum(axis=2, dtype=np.uint64) % np.uint64(q))
    return np.asarray(oracle.ntt_inverse(q, n, summed.reshape(-1, n))).reshape(batch, rows, n)


@pytest.mark.parametrize("logn", range(1, 18))
def test_matches_oracle_composition(pkg, oracle, logn):
    n, rows, cols, batch = 1 << logn, 5, 3, _batch_for(logn)
    ctx = pkg.NttContext(Q44, n, device=0)
    assert ctx.uses_f64
    rng = np.random.default_rng(2000 * logn)
    m, x = _rand(rng, Q44, (rows, cols, n)), _rand(rng, Q44, (batch, cols, n))
    mat = ctx.ring_matrix(m)
    assert np.array_equal(mat.matvec(x), _oracle_matvec(oracle, Q44, n, m, x)), n
    mat.close()
    ctx.close()


# ---- 4. row-block boundaries -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", ["f64", "u64_q60"])
def test_every_row_count_across_two_row_blocks(pkg, lib, flavour):
    n, batch, cols = 4096, 2, 2
    q, ctx = _flavour_context(pkg, lib, flavour, n)
    rng = np.random.default_rng(44 + len(flavour))
    probe = ctx.ring_matrix(np.zeros((1, 1, n), dtype=np.uint64))
    most = 2 * probe.row_block + 1
    probe.close()
    m, x = _rand(rng, q, (most, cols, n)), _rand(rng, q, (batch, cols, n))
    want = _by_ring_dot(ctx, m, x)              # row r of the product depends on row r of M alone: one reference for every row count
    for rows in range(1, most + 1):
        mat = ctx.ring_matrix(m[:rows])
        assert np.array_equal(mat.matvec(x), want[:, :rows]), (flavour, rows)
        mat.close()
    ctx.close()


# ---- 5. the accumulators: identical entries, every product of one sign per residue --------------------------------------------------
@pytest.mark.parametrize("cols", [2, 32, 33, 65, 3001])
@pytest.mark.parametrize("flavour", ["f64", "u64_q60"])
def test_accumulator_worst_case(pkg, lib, flavour, cols):
    """Every entry of M is one polynomial m0 and every column of x one polynomial x0: each of the rows' accumulators receives the same
    product cols times, so y = cols (m0 x0).  cols straddles the FP64 re-centring period (32); 3001 q / 2 > 2^54 is beyond any
    unreduced double, and 41 or more canonical 60-bit summands overflow 64 bits unless each sum is reduced.  All 3001 columns reach
    ONE launch: at n <= 4096 matvec_device is a single ntt_tile_ring_matvec launch over every column of the resident matrix.  (Which
    positions can tell a lost periodic re-centre: tests/test_f64_long_sums_gpu.py.)"""
    n = 64
    q, ctx = _flavour_context(pkg, lib, flavour, n)
    assert pkg.RING_DOT_F64_RECENTRE_PERIOD == 32
    rng = np.random.default_rng(cols)
    m0, x0 = _rand(rng, q, (n,)), _rand(rng, q, (n,))
    want = _to_u64(ctx.ring_mul(m0, x0).astype(object) * (cols % q) % q)
    x = np.ascontiguousarray(np.broadcast_to(x0, (1, cols, n)))
    probe = ctx.ring_matrix(np.zeros((1, 1, n), dtype=np.uint64))
    row_counts = sorted({2, probe.row_block})      # 2 rows, and a full block: every accumulator of a workgroup sees the worst case
    probe.close()
    for rows in row_counts:
        mat = ctx.ring_matrix(np.ascontiguousarray(np.broadcast_to(m0, (rows, cols, n))))
        got = mat.matvec(x)
        assert got.shape == (1, rows, n)
        for r in range(rows):
            assert np.array_equal(got[0, r], want), (flavour, cols, rows, r)
        mat.close()
    ctx.close()


# ---- 6. handle semantics ---------------------------------------------------------------------------------------------------------
def test_matrix_owns_its_copy(pkg):
    n, rows, cols = 256, 3, 2
    rng = np.random.default_rng(61)
    ctx = pkg.NttContext(Q_NORTH, n, device=0)
    m, x = _rand(rng, Q_NORTH, (rows, cols, n)), _rand(rng, Q_NORTH, (4, cols, n))
    want = _by_ring_dot(ctx, m, x)
    source = m.copy()
    mat = ctx.ring_matrix(source)
    source[:] = 1                                # the caller's buffer changes after create
    assert np.array_equal(mat.matvec(x), want)
    mat.close()
    ctx.close()


@pytest.mark.parametrize("n", [1024, 8192])
def test_one_matrix_on_two_streams_and_device_forms(pkg, n):
    import torch
    q, rows, cols, batch = Q44, 3, 2, 5
    rng = np.random.default_rng(62 + n)
    ctx = pkg.NttContext(q, n, device=0)
    m = _rand(rng, q, (rows, cols, n))
    xa, xb = _rand(rng, q, (batch, cols, n)), _rand(rng, q, (batch, cols, n))
    host_mat = ctx.ring_matrix(m)
    want_a, want_b = host_mat.matvec(xa), host_mat.matvec(xb)
    assert np.array_equal(want_a, _by_ring_dot(ctx, m, xa))
    d_m, d_xa, d_xb = _dev(torch, m), _dev(torch, xa), _dev(torch, xb)
    ya = torch.empty((batch, rows, n), dtype=torch.int64, device="cuda")
    yb, yc = torch.empty_like(ya), torch.empty_like(ya)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    dev_mat = ctx.ring_matrix_device(d_m.data_ptr(), rows, cols, s1.cuda_stream)
    assert (dev_mat.rows, dev_mat.cols, dev_mat.row_block) == (rows, cols, host_mat.row_block)
    # the device-created matrix on two streams, no synchronisation between create and the calls
    dev_mat.matvec_device(ya.data_ptr(), d_xa.data_ptr(), batch, s1.cuda_stream)
    dev_mat.matvec_device(yb.data_ptr(), d_xb.data_ptr(), batch, s2.cuda_stream)
    # the device entry on the host-created matrix
    host_mat.matvec_device(yc.data_ptr(), d_xb.data_ptr(), batch, s2.cuda_stream)
    s1.synchronize()
    s2.synchronize()
    assert np.array_equal(_host(ya), want_a)
    assert np.array_equal(_host(yb), want_b)
    assert np.array_equal(_host(yc), want_b)
    assert np.array_equal(dev_mat.matvec(xa), want_a)
    dev_mat.close()
    host_mat.close()
    ctx.close()


def test_composed_route_beside_ring_dot_from_another_thread(pkg):
    """n = 8192: the mat-vec goes through the context's ring workspace.  One thread issues mat-vecs on its stream while another issues
    ring inner products on the same context on another stream; every call of either kind must see the workspace to itself."""
    import threading
    import torch
    q, n, rows, cols, batch, rounds = Q44, 8192, 3, 2, 4, 4
    rng = np.random.default_rng(63)
    ctx = pkg.NttContext(q, n, device=0)
    m, x = _rand(rng, q, (rows, cols, n)), _rand(rng, q, (batch, cols, n))
    a, b = _rand(rng, q, (batch, cols, n)), _rand(rng, q, (batch, cols, n))
    mat = ctx.ring_matrix(m)
    want_y, want_c = mat.matvec(x), ctx.ring_dot(a, b)
    d_x, d_a, d_b = _dev(torch, x), _dev(torch, a), _dev(torch, b)
    ys = [torch.empty((batch, rows, n), dtype=torch.int64, device="cuda") for _ in range(rounds)]
    cs = [torch.empty((batch, n), dtype=torch.int64, device="cuda") for _ in range(rounds)]
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    errors = []

    def run(fn):
        try:
            for i in range(rounds):
                fn(i)
        except Exception as e:      # noqa: BLE001 (reported below)
            errors.append(e)

    t1 = threading.Thread(target=run, args=(lambda i: mat.matvec_device(ys[i].data_ptr(), d_x.data_ptr(), batch, s1.cuda_stream),))
    t2 = threading.Thread(target=run, args=(lambda i: ctx.ring_dot_device(cs[i].data_ptr(), d_a.data_ptr(), d_b.data_ptr(), batch, cols, batch, s2.cuda_stream),))
    t1.start()
    t2.start()
    t1.join()
    t2.join()
    s1.synchronize()
    s2.synchronize()
    assert not errors, errors
    for i in range(rounds):
        assert np.array_equal(_host(ys[i]), want_y), i
        assert np.array_equal(_host(cs[i]), want_c), i
    mat.close()
    ctx.close()


# ---- 7. refusals on a real context -----------------------------------------------------------------------------------------------
def test_output_overlapping_the_operand_is_refused(pkg):
    import torch
    n, rows, cols, batch = 256, 3, 2, 2
    rng = np.random.default_rng(71)
    ctx = pkg.NttContext(Q_NORTH, n, device=0)
    m = _rand(rng, Q_NORTH, (rows, cols, n))
    mat = ctx.ring_matrix(m)
    buf = torch.zeros((batch * cols + batch * rows, n), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    fn = ctx._lib.lsr_ntt_ring_matvec_batch_device
    # y straddling the operand's end / y on the operand's first rows / y right behind the operand (allowed)
    for y_row, rc_want in [(batch * cols - 1, -1), (0, -1), (batch * cols, 0)]:
        assert fn(mat.handle, buf[y_row].data_ptr(), buf.data_ptr(), batch, _stream(torch)) == rc_want, y_row
        assert rc_want == 0 or "y overlaps x" in pkg._abi.last_error()
    torch.cuda.synchronize()
    host = np.zeros((batch * cols + batch * rows, n), dtype=np.uint64)
    assert ctx._lib.lsr_ntt_ring_matvec_batch(mat.handle, host[1].ctypes.data, host.ctypes.data, batch) == -1
    assert "y overlaps x" in pkg._abi.last_error()
    x = _rand(rng, Q_NORTH, (batch, cols, n))    # the matrix and the context still work
    assert np.array_equal(mat.matvec(x), _by_ring_dot(ctx, m, x))
    mat.close()
    ctx.close()


def test_context_above_two_pass_sizes_is_refused(pkg):
    ntt = pkg.CyclicNtt(1 << 18)
    with pytest.raises(pkg.CoreError):
        ntt.ring_matrix(np.zeros((1, 1, 1 << 18), dtype=np.uint64))
    assert "131072" in pkg._abi.last_error()
    ntt.close()


def test_matrix_above_the_byte_cap_is_refused(pkg):
    """Within the caps on rows and cols, over LSR_RING_MATVEC_MAX_MATRIX_BYTES at this n only: refused before the buffer is read."""
    import ctypes
    n = 4096
    ctx = pkg.NttContext(Q_NORTH, n, device=0)
    rows, cols = 129, pkg.RING_MATVEC_MAX_MATRIX_BYTES // (n * 8) // 128
    assert rows * cols * 16 <= pkg.RING_MATVEC_MAX_MATRIX_BYTES < rows * cols * n * 8
    word = (ctypes.c_uint64 * 1)()
    assert not ctx._lib.lsr_ntt_ring_matrix_create(ctx.handle, ctypes.addressof(word), rows, cols)
    assert "LSR_RING_MATVEC_MAX_MATRIX_BYTES" in pkg._abi.last_error()
    ctx.close()
