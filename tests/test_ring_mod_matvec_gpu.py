"""GPU suite: resident-matrix products under an arbitrary modulus (RingMod.matrix* / RingModMatrix: lsr_ring_mod_matrix_* and
lsr_ring_mod_matvec_*, batch.h) against the Python-integer model (tests/ring_mod_matvec_model.py), against the handle's
own fused inner product and multiply, and against the single-prime resident matrix where q happens to be an NTT prime.  Every
comparison is exact, word for word.  Shapes are the smallest at which each mechanism can fail: rows 5 (one full row block of 4 and a
ragged one), batch 5 (a partial tile below n = 4096), cols above max_terms (column groups reduced with accumulate), a gadget group
that ends between two digits of one column, one vector past a workspace chunk, one row past a row range."""
import functools

import numpy as np
import pytest

import ring_gadget_model as gadget
import ring_mod_matvec_model as model
import ring_mod_model as mod

pytestmark = pytest.mark.gpu

P5 = mod.prime_5_mod_8_below(1 << 32)
Q40 = (1 << 40) + 15                       # odd, 41 bits: max_terms = 7 at n = 64
ROWS, COLS, BATCH = 5, 3, 5
SUM_WORDS = 1 << 22                        # the handle's workspace per prime


def _dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.uint64)).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _random(rng, q, shape):
    return rng.integers(0, q, size=shape, dtype=np.uint64)


def _with_extremes(x, q):
    """the centred extremes floor(q/2) and floor(q/2) + 1 in whole polynomials"""
    x[0, 0, :] = q // 2
    x[1, 0, :] = min(q // 2 + 1, q - 1)
    return x


def _matvec_device(torch, mat, x, gadget_args=None):
    """matvec_device / matvec_gadget_device on a numpy x [batch][xcols][n] -> numpy y [batch][rows][n]"""
    d_x = _dev(torch, x)
    d_y = torch.full((x.shape[0], mat.rows, mat.n), -1, dtype=torch.int64, device="cuda")
    if gadget_args is None:
        mat.matvec_device(d_y.data_ptr(), d_x.data_ptr(), x.shape[0], stream=_stream(torch))
    else:
        mat.matvec_gadget_device(d_y.data_ptr(), d_x.data_ptr(), x.shape[0], *gadget_args, stream=_stream(torch))
    torch.cuda.synchronize()
    return _host(d_y)


@functools.lru_cache(maxsize=None)
def _plain_reference(n, q, rows=ROWS, cols=COLS, batch=BATCH):
    rng = np.random.default_rng(7000 * n + q % 991 + cols)
    m, x = _random(rng, q, (rows, cols, n)), _with_extremes(_random(rng, q, (batch, cols, n)), q)
    want = model.matvec(m, x, q)
    want.setflags(write=False)
    return m, x, want


# ---- 1. model parity, plain ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,q", [(2, 2), (4, 3329), (64, P5), (256, 3329), (64, 1 << 32)])
def test_plain_product_equals_the_model(pkg, n, q):
    import torch
    m, x, want = _plain_reference(n, q)
    with pkg.RingMod(q, n, device=0) as ring:
        with ring.matrix(m) as mat:
            assert (mat.rows, mat.cols) == (ROWS, COLS) and mat.row_block in (2, 4)
            assert np.array_equal(mat.matvec(x), want)                                        # host form
            assert np.array_equal(mat.matvec(x[0]), want[0])
            assert np.array_equal(_matvec_device(torch, mat, x), want)                        # device form
        with ring.matrix_device(_dev(torch, m).data_ptr(), ROWS, COLS, stream=_stream(torch)) as mat:
            assert np.array_equal(_matvec_device(torch, mat, x), want)


# ---- 2. column groups ------------------------------------------------------------------------------------------------------------
def test_column_groups_above_max_terms(pkg):
    """cols 17 at max_terms 7: groups of 7, 7 and 3"""
    import torch
    n, q, cols = 64, Q40, 17
    assert mod.capacity(q, n) == 7
    m, x, want = _plain_reference(n, q, cols=cols)
    with pkg.RingMod(q, n, device=0) as ring, ring.matrix(m) as mat:
        assert ring.max_terms == 7
        got = _matvec_device(torch, mat, x)
        assert np.array_equal(got, want)
        assert np.array_equal(mat.matvec(x), want)
        d_x, d_c = _dev(torch, x), torch.empty((BATCH, n), dtype=torch.int64, device="cuda")
        for r in range(ROWS):                                                               # the handle's own inner product, row by row
            d_b = _dev(torch, m[r])
            ring.dot_device(d_c.data_ptr(), d_x.data_ptr(), d_b.data_ptr(), BATCH, cols, 1, stream=_stream(torch))
            torch.cuda.synchronize()
            assert np.array_equal(got[:, r], _host(d_c)), r


# ---- 3. gadget against the model and against the plain product on the model's decomposition ---------------------------------------
@pytest.mark.parametrize("n,q,b", [(64, P5, 11), (256, 3329, 4), (64, Q40, 8)])
def test_gadget_product_equals_the_model_and_the_plain_product_on_the_digits(pkg, lib, n, q, b):
    import torch
    digits, xcols = int(lib.lsr_ring_gadget_min_digits(q, b)), 3
    assert digits == gadget.min_digits(q, b) >= 1
    cols = xcols * digits
    rng = np.random.default_rng(n + b)
    m, x = _random(rng, q, (ROWS, cols, n)), _with_extremes(_random(rng, q, (BATCH, xcols, n)), q)
    z = model.decomposed(x, q, b, digits)
    want = model.matvec(m, z, q)
    assert np.array_equal(want, model.matvec_gadget(m, x, q, b, digits))
    if q == Q40:                                    # one group where the plain product runs three
        assert pkg.ring_mod_capacity_bounded(q, n, 1 << (b - 1)) >= cols > 2 * pkg.ring_mod_capacity(q, n)
    with pkg.RingMod(q, n, device=0) as ring, ring.matrix(m) as mat:
        assert np.array_equal(_matvec_device(torch, mat, x, (b, digits)), want)
        assert np.array_equal(mat.matvec_gadget(x, b, digits), want)
        assert np.array_equal(_matvec_device(torch, mat, z), want)


# ---- 4. gadget groups that split a column ------------------------------------------------------------------------------------------
def test_gadget_group_boundary_between_two_digits_of_one_column(pkg, lib):
    """capacity 2047 is odd and D = 2: the first group ends between the two digits of x column 1023"""
    import torch
    n, q, b, digits, xcols, rows, batch = 64, Q40, 32, 2, 1025, 1, 2
    assert gadget.admissible(q, b, digits) and int(lib.lsr_ring_gadget_min_digits(q, b)) == digits
    assert pkg.ring_mod_capacity_bounded(q, n, 1 << 31) == 2047 == model.capacity_bounded(q, n, 1 << 31)
    rng = np.random.default_rng(2047)
    m, x = _random(rng, q, (rows, xcols * digits, n)), _with_extremes(_random(rng, q, (batch, xcols, n)), q)
    want = model.matvec_gadget(m, x, q, b, digits)
    with pkg.RingMod(q, n, device=0) as ring, ring.matrix(m) as mat:
        assert np.array_equal(_matvec_device(torch, mat, x, (b, digits)), want)


# ---- 5. n = 4096 -------------------------------------------------------------------------------------------------------------------
def test_n_4096_on_sampled_coefficients(pkg):
    import torch
    n, q, rows, cols, batch = 4096, 1 << 32, 3, 2, 2
    rng = np.random.default_rng(4096)
    m, x = _random(rng, q, (rows, cols, n)), _random(rng, q, (batch, cols, n))
    positions = sorted({0, 1, n // 2, n - 2, n - 1} | set(rng.integers(0, n, size=59).tolist()))
    with pkg.RingMod(q, n, device=0) as ring, ring.matrix(m) as mat:
        got = _matvec_device(torch, mat, x)
        for j in range(batch):
            for r in range(rows):
                assert [int(got[j, r, k]) for k in positions] == [model.matvec_coefficient(m, x, q, j, r, k) for k in positions], (j, r)


# ---- 6. vector chunks --------------------------------------------------------------------------------------------------------------
def test_one_vector_past_a_workspace_chunk(pkg):
    import torch
    n, q, rows, cols = 64, P5, 5, 2
    batch = SUM_WORDS // (rows * n) + 1
    rng = np.random.default_rng(66)
    m = _random(rng, q, (rows, cols, n))
    d_x = _dev(torch, _random(rng, q, (batch, cols, n)))
    d_y = torch.full((batch, rows, n), -1, dtype=torch.int64, device="cuda")
    d_c = torch.empty((batch, n), dtype=torch.int64, device="cuda")
    with pkg.RingMod(q, n, device=0) as ring, ring.matrix(m) as mat:
        mat.matvec_device(d_y.data_ptr(), d_x.data_ptr(), batch, stream=_stream(torch))
        for r in range(rows):
            d_b = _dev(torch, m[r])
            ring.dot_device(d_c.data_ptr(), d_x.data_ptr(), d_b.data_ptr(), batch, cols, 1, stream=_stream(torch))
            assert torch.equal(d_y[:, r], d_c), r
        torch.cuda.synchronize()


# ---- 7. row ranges -----------------------------------------------------------------------------------------------------------------
def test_one_row_past_a_row_range(pkg):
    """rows n above the workspace: one vector and 1024 rows at a time, then the last row"""
    import torch
    n, q, rows, batch = 4096, 1 << 32, SUM_WORDS // 4096 + 1, 2
    rng = np.random.default_rng(1025)
    d_m = _dev(torch, _random(rng, q, (rows, 1, n)))
    d_x = _dev(torch, _random(rng, q, (batch, 1, n)))
    d_y = torch.full((batch, rows, n), -1, dtype=torch.int64, device="cuda")
    d_c = torch.empty((rows, n), dtype=torch.int64, device="cuda")
    with pkg.RingMod(q, n, device=0) as ring, ring.matrix_device(d_m.data_ptr(), rows, 1, stream=_stream(torch)) as mat:
        mat.matvec_device(d_y.data_ptr(), d_x.data_ptr(), batch, stream=_stream(torch))
        for j in range(batch):                                                               # M[r][0] x[j] for every r: x[j] the shared operand
            ring.mul_device(d_c.data_ptr(), d_m.data_ptr(), d_x[j].data_ptr(), rows, 1, stream=_stream(torch))
            assert torch.equal(d_y[j], d_c), j
        torch.cuda.synchronize()


# ---- 8. seeded ---------------------------------------------------------------------------------------------------------------------
def test_seeded_matrix_is_the_matrix_of_the_models_words(pkg, oracle):
    import torch
    import ring_sample_model
    n, q, rows, cols, domain, base = 64, P5, 3, 2, 21, 11
    key = pkg.ring_sample_key(5)
    words = model.seeded_matrix(oracle, q, n, ring_sample_model.key_from_seed(5), domain, base, rows, cols)
    assert words.max() < q
    units = np.zeros((cols, cols, n), dtype=np.uint64)
    for c in range(cols):
        units[c, c, 0] = 1                                                                  # x[c] = the unit vector e_c
    rng = np.random.default_rng(8)
    x = _random(rng, q, (BATCH, cols, n))
    with pkg.RingMod(q, n, device=0) as ring, ring.matrix_seeded(key, domain, base, rows, cols) as seeded:
        assert (seeded.rows, seeded.cols) == (rows, cols)
        got = _matvec_device(torch, seeded, units)                                          # [c][r] = M[r][c]
        assert np.array_equal(np.transpose(got, (1, 0, 2)), words)
        with ring.matrix_device(_dev(torch, words).data_ptr(), rows, cols, stream=_stream(torch)) as plain:
            assert np.array_equal(_matvec_device(torch, seeded, x), _matvec_device(torch, plain, x))
            assert seeded.row_block == plain.row_block


# ---- 9. capture --------------------------------------------------------------------------------------------------------------------
def test_graph_capture_straight_after_create(pkg):
    """no eager product first: the workspace exists since the handle's create.  Both products in one graph; two replays."""
    import torch
    n, q, b, rows, xcols = 64, Q40, 8, ROWS, 3
    digits = gadget.min_digits(q, b)
    cols = xcols * digits
    assert cols > 2 * mod.capacity(q, n)                                                      # the plain product runs three groups
    rng = np.random.default_rng(99)
    m = _random(rng, q, (rows, cols, n))
    ring = pkg.RingMod(q, n, device=0)
    mat = ring.matrix_device(_dev(torch, m).data_ptr(), rows, cols, stream=_stream(torch))
    d_x = torch.zeros((BATCH, cols, n), dtype=torch.int64, device="cuda")
    d_xg = torch.zeros((BATCH, xcols, n), dtype=torch.int64, device="cuda")
    d_y = [torch.empty((BATCH, rows, n), dtype=torch.int64, device="cuda") for _ in range(2)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        mat.matvec_device(d_y[0].data_ptr(), d_x.data_ptr(), BATCH, stream=torch.cuda.current_stream().cuda_stream)
        mat.matvec_gadget_device(d_y[1].data_ptr(), d_xg.data_ptr(), BATCH, b, digits, stream=torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        x, xg = _random(rng, q, (BATCH, cols, n)), _random(rng, q, (BATCH, xcols, n))
        d_x.copy_(_dev(torch, x))
        d_xg.copy_(_dev(torch, xg))
        graph.replay()
        torch.cuda.synchronize()
        replayed = [_host(d).copy() for d in d_y]
        assert np.array_equal(replayed[0], _matvec_device(torch, mat, x))                    # the eager results
        assert np.array_equal(replayed[1], _matvec_device(torch, mat, xg, (b, digits)))
    assert np.array_equal(replayed[0], model.matvec(m, x, q))
    mat.close()
    ring.close()                               # free while idle


# ---- the integer flavour of the prime contexts ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 2048])
def test_integer_flavour_equals_the_fp64_flavour(pkg, lib, n):
    """a process that forces the integer kernels: row blocks of 2, and at n = 2048 the gadget product launches once per prime.  Both
    flavours are held to the model as well as to each other: a mistake they share (the loader, the column-range addressing, the
    reduce pass) does not cancel."""
    import torch
    q, b, xcols, batch = P5, 8, 3, 3                                                         # (2^40 + 15 is not admissible at n = 2048)
    digits = gadget.min_digits(q, b)
    cols = xcols * digits
    assert mod.capacity(q, n) >= 1 and digits >= 4
    rng = np.random.default_rng(n + 11)
    m = _random(rng, q, (ROWS, cols, n))
    x, xg = _with_extremes(_random(rng, q, (batch, cols, n)), q), _with_extremes(_random(rng, q, (batch, xcols, n)), q)
    want, want_gadget = model.matvec(m, x, q), model.matvec_gadget(m, xg, q, b, digits)
    lib.lsr_set_arith_mode(1)
    try:
        integer = pkg.RingMod(q, n, device=0)
    finally:
        lib.lsr_set_arith_mode(0)
    with integer, pkg.RingMod(q, n, device=0) as fp64:
        assert not integer.prime_context(0).uses_f64 and fp64.prime_context(0).uses_f64
        with integer.matrix(m) as mi, fp64.matrix(m) as mf:
            assert (mi.row_block, mf.row_block) == (2, 4)
            assert np.array_equal(_matvec_device(torch, mi, x), _matvec_device(torch, mf, x))
            assert np.array_equal(_matvec_device(torch, mi, xg, (b, digits)), _matvec_device(torch, mf, xg, (b, digits)))
            for name, mat in (("integer", mi), ("fp64", mf)):
                assert np.array_equal(_matvec_device(torch, mat, x), want), name
                assert np.array_equal(_matvec_device(torch, mat, xg, (b, digits)), want_gadget), name


# ---- 10. an NTT prime the handle admits ---------------------------------------------------------------------------------------------
def _ntt_prime_for(n):
    """p1 of degree n where the handle admits it, else the largest prime = 1 (mod 2n) it admits"""
    p1 = mod.primes(n)[0]
    if mod.capacity(p1, n) >= 1:
        return p1
    cand = (mod.largest_admissible(n) - 1) // (2 * n) * (2 * n) + 1
    while not mod.is_prime(cand):
        cand -= 2 * n
    return cand


@pytest.mark.parametrize("n", [64, 4096])
def test_products_equal_the_single_prime_matrix_at_an_ntt_prime(pkg, n):
    import torch
    q, b, xcols, rows, batch = _ntt_prime_for(n), 11, 2, ROWS, 3
    assert mod.capacity(q, n) >= 1 and q % (2 * n) == 1
    digits = gadget.min_digits(q, b)
    cols = xcols * digits
    rng = np.random.default_rng(n + 10)
    d_m = _dev(torch, _random(rng, q, (rows, cols, n)))
    x, xg = _random(rng, q, (batch, cols, n)), _with_extremes(_random(rng, q, (batch, xcols, n)), q)
    with pkg.RingMod(q, n, device=0) as ring, pkg.NttContext(q, n, device=0) as ctx:
        with ring.matrix_device(d_m.data_ptr(), rows, cols, stream=_stream(torch)) as mat, \
                ctx.ring_matrix_device(d_m.data_ptr(), rows, cols, stream=_stream(torch)) as single:
            assert np.array_equal(_matvec_device(torch, mat, x), _matvec_device(torch, single, x))
            assert np.array_equal(_matvec_device(torch, mat, xg, (b, digits)), _matvec_device(torch, single, xg, (b, digits)))
