"""GPU suite: the exact l2 norm, the seeded Johnson-Lindenstrauss projection and the rows of its matrix (lsr_ntt_ring_l2sq_batch,
lsr_ntt_ring_project_batch, lsr_ntt_ring_project_matrix_batch and their _device forms) word for word against the
Python-integer model of tests/ring_norm_model.py, in the host and the device form, on every kind of context; at the accumulator
bound; in the three statuses and the saturation of the norm; against the existing twisted inner product; in the refusals that read
the context; and under graph capture with no warm-up call."""
import numpy as np
import pytest

import ring_norm_model as model
from ring_norm_model import ROWS, SATURATED, key_from_bytes, key_from_seed
from test_ring_matvec_gpu import _flavour_context

pytestmark = pytest.mark.gpu

Q14 = 12289
Q44 = 17592180539393           # 44-bit prime, 2^18 | q - 1: every n up to 2^17
Q60 = 1152921504606584833
GOLD = 18446744069414584321
SLICE = 2048                   # kProjectSlice of lsr_ring_norm_kernels.hpp: the positions of one workgroup
# (n, width): less than one stream word; len 40 crosses a word and ends inside one; a ragged block; two slices; 2.5 slices; 32 slices
SHAPES = [(2, 1), (8, 5), (256, 3), (1024, 5), (4096, 2), (65536, 1)]
CONTEXTS = ["q14", "f64", "u64_q44", "u64_q60", "gold"]


def _context(pkg, lib, kind, n):
    if kind == "q14":
        return Q14, pkg.NttContext(Q14, n, device=0)
    if kind == "gold":
        return GOLD, pkg.CyclicNtt(n)
    return _flavour_context(pkg, lib, kind, n)


def _dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()


def _keys_array(keys):
    return np.array(keys, dtype=np.uint64)


def _short(rng, q, bound, shape):
    """Canonical words whose centred values are uniform on [-bound, bound]."""
    v = rng.integers(-bound, bound + 1, size=shape, dtype=np.int64).astype(object)
    return np.array(v % q, dtype=np.uint64)


def _l2_words(values):
    return [[v & (2**64 - 1), v >> 64] for v in values]


def _check_all_forms(pkg, oracle, ctx, q, n, width, count, keys, components, index_base, seed, matrix_rows):
    """project and l2sq of one batch in the host and the device form, and rows of the first key's matrix, against the model."""
    import torch
    rng = np.random.default_rng(seed)
    length = width * n
    bound = min(q // 2, (2**63 - 1) // length, 1 << 62)
    x = _short(rng, q, bound, (count, width, n))
    want, want_status = model.project(oracle, q, x, bound, keys, components, 17, index_base)
    assert want_status.tolist() == [1] * count
    want_l2 = model.l2sq(q, x)
    karr = _keys_array(keys)

    got, status = ctx.ring_project(x, bound, karr, components=components, index_base=index_base)
    assert status.tolist() == [1] * count and got.dtype == np.int64
    assert np.array_equal(got, want), (q, n, width)
    l2 = ctx.ring_l2sq(x)
    assert l2.tolist() == want_l2 and all(isinstance(v, int) for v in l2.tolist())

    d_x, d_keys = _dev(torch, x), _dev(torch, karr)
    d_out = torch.full((count, ROWS), -1, dtype=torch.int64, device="cuda")
    d_status = torch.full((count,), 7, dtype=torch.int32, device="cuda")
    d_l2 = torch.zeros((count, 2), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.current_stream().cuda_stream
    ctx.ring_project_device(d_out.data_ptr(), d_status.data_ptr(), d_x.data_ptr(), count, width, bound, d_keys.data_ptr(), components, 17, index_base, s)
    ctx.ring_l2sq_device(d_x.data_ptr(), count, width, d_l2.data_ptr(), s)
    torch.cuda.current_stream().synchronize()
    assert np.array_equal(d_out.cpu().numpy(), want) and d_status.cpu().tolist() == [1] * count
    assert d_l2.cpu().numpy().view(np.uint64).tolist() == _l2_words(want_l2)

    first, rows = matrix_rows
    want_m = model.project_matrix(oracle, q, n, width, keys[0], first, rows, 17, index_base)
    assert np.array_equal(ctx.ring_project_matrix(karr[0], width, first, rows, index_base=index_base), want_m)
    d_m = torch.zeros((rows, width, n), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.ring_project_matrix_device(d_m.data_ptr(), first, rows, width, d_keys.data_ptr(), 17, index_base, s)
    torch.cuda.current_stream().synchronize()
    assert np.array_equal(d_m.cpu().numpy().view(np.uint64), want_m)


# ---- 1. word for word against the model ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", CONTEXTS)
@pytest.mark.parametrize("n,width", SHAPES)
def test_matches_the_model(pkg, lib, oracle, kind, n, width):
    """count 5 with components 2: a ragged last group, three keys (the middle one from bytes), index_base != 0.  The two longest
    shapes take two vectors under seed keys (the model reads a byte key block by block).  Q14 has no ring above n = 2048: there the
    two long shapes keep their lengths at n = 2048."""
    assert (width * n > 2 * SLICE and (width * n) % SLICE != 0) == ((n, width) == (1024, 5))
    if kind == "q14" and n > 2048:
        n, width = 2048, n * width // 2048
    q, ctx = _context(pkg, lib, kind, n)
    if width * n <= 1024:
        keys = [key_from_seed(n + 1), key_from_bytes(bytes(range(7, 39))), key_from_seed(n + 2)]
        _check_all_forms(pkg, oracle, ctx, q, n, width, 5, keys, 2, 7, n + width, (0, ROWS))
    elif width * n <= 8192:
        keys = [key_from_seed(n + 1), key_from_seed(n + 2), key_from_seed(n + 3)]
        _check_all_forms(pkg, oracle, ctx, q, n, width, 5, keys, 2, (1 << 40) + 3, n + width, (250, 6))
    else:
        _check_all_forms(pkg, oracle, ctx, q, n, width, 2, [key_from_seed(n + 1), key_from_seed(n + 2)], 1, 0, n + width, (254, 2))
    ctx.close()


def test_large_cyclic_context_matches_the_model(pkg, oracle):
    n = 1 << 18                                                   # the smallest n above 2^17
    ntt = pkg.CyclicNtt(n)
    _check_all_forms(pkg, oracle, ntt, GOLD, n, 1, 2, [key_from_seed(18)], 2, 5, 18, (255, 1))
    ntt.close()


# ---- 2. planted cases ------------------------------------------------------------------------------------------------------------------
def test_projection_at_the_accumulator_bound(pkg, oracle):
    """Q60, n = 8, width 1, every coefficient +floor(q/2), then -floor(q/2), under the largest bound there is, floor(q/2): sums of up
    to 2^62, far beyond what a float64 accumulator holds exactly."""
    q, n = Q60, 8
    ctx = pkg.NttContext(q, n, device=0)
    key = key_from_seed(60)
    for v in (q // 2, q - q // 2):
        x = np.full((1, 1, n), v, dtype=np.uint64)
        want = model.project_ints(oracle, q, x.reshape(-1).tolist(), key)
        got, status = ctx.ring_project(x, q // 2, _keys_array([key]))
        assert status.tolist() == [1] and got[0].tolist() == want
        assert max(abs(p) for p in want) > 2**60
    ctx.close()


@pytest.mark.parametrize("kind,n,width", [("f64", 256, 3), ("u64_q60", 4096, 2), ("gold", 8, 5)])
def test_statuses_leave_the_neighbours_alone(pkg, lib, oracle, kind, n, width):
    """Vector 1 has one coefficient of |v| = bound + 1 (status 0), vector 3 a word = q (-1), vector 4 both (-1); the bad words sit
    in the last slice of their vector.  Vectors 0 and 2 are served as if alone."""
    import torch
    q, ctx = _context(pkg, lib, kind, n)
    rng = np.random.default_rng(n + width)
    bound = 1000
    x = _short(rng, q, bound, (5, width, n))
    x[1, width - 1, n - 3] = q - (bound + 1)
    x[3, width - 1, n - 1] = q
    x[4, 0, 0] = bound + 1
    x[4, width - 1, n - 2] = 2**64 - 1
    keys = [key_from_seed(5)]
    want, want_status = model.project(oracle, q, x, bound, keys, 5)
    assert want_status.tolist() == [1, 0, 1, -1, -1] and not want[[1, 3, 4]].any() and want[0].any() and want[2].any()
    got, status = ctx.ring_project(x, bound, _keys_array(keys), components=5)
    assert status.tolist() == want_status.tolist() and np.array_equal(got, want)
    x[1, width - 1, n - 3] = q - bound                            # exactly at the bound: served
    assert ctx.ring_project(x[1], bound, _keys_array(keys), components=5, index_base=ROWS)[1] == 1
    d_x, d_keys = _dev(torch, x), _dev(torch, _keys_array(keys))
    d_out = torch.full((5, ROWS), -1, dtype=torch.int64, device="cuda")
    d_status = torch.full((5,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.ring_project_device(d_out.data_ptr(), d_status.data_ptr(), d_x.data_ptr(), 5, width, bound, d_keys.data_ptr(), 5, 17, 0,
                            torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    want2, want_status2 = model.project(oracle, q, x, bound, keys, 5)
    assert want_status2.tolist() == [1, 1, 1, -1, -1]
    assert d_status.cpu().tolist() == want_status2.tolist() and np.array_equal(d_out.cpu().numpy(), want2)
    # the norm: all ones for the vectors with a word >= q, the neighbours exact
    l2 = ctx.ring_l2sq(x)
    assert l2.tolist() == model.l2sq(q, x) and l2[3] == l2[4] == SATURATED and max(l2[:3]) < SATURATED
    ctx.close()


def test_l2_saturates_exactly_at_the_top(pkg):
    for q, n, make in [(Q60, 1024, lambda n: pkg.NttContext(Q60, n, device=0)), (GOLD, 4, lambda n: pkg.CyclicNtt(n))]:
        ctx = make(n)
        one = np.full((1, 1, n), q // 2, dtype=np.uint64)
        exact = n * (q // 2) ** 2
        assert 2**127 < exact < SATURATED <= 2 * exact
        assert ctx.ring_l2sq(one).tolist() == [exact] and ctx.ring_l2sq(one[0]) == exact
        if q == Q60:                                             # width 2 at the same n
            assert ctx.ring_l2sq(np.full((1, 2, n), q // 2, dtype=np.uint64)).tolist() == [SATURATED]
            both = np.full((3, 2, n), q // 2, dtype=np.uint64)   # a saturated vector between two exact ones
            both[0, 1] = 0
            both[2, 0] = 0
            assert ctx.ring_l2sq(both).tolist() == [exact, SATURATED, exact]
        ctx.close()
    ctx = pkg.CyclicNtt(8)                                       # Goldilocks: n = 8 saturates
    assert ctx.ring_l2sq(np.full((1, 1, 8), GOLD // 2, dtype=np.uint64)).tolist() == [SATURATED]
    x = np.full((2, 1, 8), GOLD - GOLD // 2, dtype=np.uint64)    # -floor(q/2): the same squares
    x[1, 0, 4:] = 0
    assert ctx.ring_l2sq(x).tolist() == [SATURATED, 4 * (GOLD // 2) ** 2]
    ctx.close()


# ---- 3. the cross-check with the twisted inner product ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n,width", [(256, 3), (4096, 2)])
def test_matrix_rows_prove_the_projection_mod_q(pkg, oracle, n, width):
    """Coefficient 0 of sum_c conj(pi_r[c]) s[c] is <pi_r, s> mod q: computed by code that shares nothing with the projection."""
    q = Q44
    ctx = pkg.NttContext(q, n, device=0)
    rng = np.random.default_rng(n)
    bound = 1 << 20
    s = _short(rng, q, bound, (1, width, n))
    key = _keys_array([key_from_seed(n + 44)])
    p, status = ctx.ring_project(s, bound, key, index_base=9)
    assert status.tolist() == [1] and p.any()
    rows = [0, 1, 100, 254, 255]
    for r in rows:
        row = ctx.ring_project_matrix(key, width, r, 1, index_base=9)
        assert set(np.unique(row).tolist()) == {0, 1, q - 1}
        dot = ctx.ring_dot_galois(row, s, ctx.galois_conjugation)
        assert int(dot[0, 0]) == int(p[0, r]) % q, r
    ctx.close()


# ---- 4. the refusals that read the context ---------------------------------------------------------------------------------------------
def test_context_rules_are_refused(pkg):
    q, n = Q60, 8
    ctx = pkg.NttContext(q, n, device=0)
    key = _keys_array([key_from_seed(1)])
    x = np.zeros((1, 1, n), dtype=np.uint64)
    for bound, width, index_base, components, needle in [
            (q // 2 + 1, 1, 0, 1, "floor(q / 2)"),                # above floor(q/2) (reported before the product rule)
            (q // 2, 3, 0, 1, "2^63 - 1"),                        # 24 * floor(q/2) does not fit (16 * floor(q/2) = 2^63 - 2^21 does)
            (1, 1, 2**64 - 256, 1, "index_base"),                 # index_base + 256 wraps
            (1, 1, 0, 2**56, "index_base")]:                      # 256 * components wraps
        xs = np.zeros((1, width, n), dtype=np.uint64)
        with pytest.raises(pkg.CoreError):
            ctx.ring_project(xs, bound, key, components=components, index_base=index_base)
        msg = pkg._abi.last_error()
        assert needle in msg and "lsr_ntt_ring_project_batch:" in msg, msg
    assert ctx.ring_project(x, q // 2, key, index_base=2**64 - 257)[1].tolist() == [1]      # the last index that fits
    with pytest.raises(pkg.CoreError):
        ctx.ring_project_matrix(key, 1, index_base=2**64 - 255)
    assert "index_base" in pkg._abi.last_error()
    # the outputs may not share memory with the operand
    buf = np.zeros((2, ROWS), dtype=np.uint64)
    status = np.zeros(2, dtype=np.int32)
    lib = ctx._lib
    assert lib.lsr_ntt_ring_project_batch(ctx.handle, buf.ctypes.data, status.ctypes.data, buf.ctypes.data, 1, 1, 1, key.ctypes.data, 1, 17, 0) == -1
    assert "out overlaps x" in pkg._abi.last_error()
    assert lib.lsr_ntt_ring_l2sq_batch(ctx.handle, buf.ctypes.data, 1, 1, buf.ctypes.data) == -1
    assert "out overlaps x" in pkg._abi.last_error() and "lsr_ntt_ring_l2sq_batch:" in pkg._abi.last_error()
    ctx.close()


# ---- 5. graph capture with no warm-up call ---------------------------------------------------------------------------------------------
def test_graph_capture_from_the_first_call(pkg, oracle):
    """The first calls this context ever sees are the captured ones; two replays on fresh inputs equal the eager results."""
    import torch
    q, n, width, count, bound = Q44, 1024, 5, 3, 1 << 20
    ctx = pkg.NttContext(q, n, device=0)
    rng = np.random.default_rng(1024)
    keys = _keys_array([key_from_seed(71), key_from_seed(72)])
    d_keys = _dev(torch, keys)
    d_x = torch.zeros((count, width, n), dtype=torch.int64, device="cuda")
    d_out = torch.full((count, ROWS), -1, dtype=torch.int64, device="cuda")
    d_status = torch.full((count,), 7, dtype=torch.int32, device="cuda")
    d_l2 = torch.zeros((count, 2), dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        s = torch.cuda.current_stream().cuda_stream
        ctx.ring_project_device(d_out.data_ptr(), d_status.data_ptr(), d_x.data_ptr(), count, width, bound, d_keys.data_ptr(), 2, 17, 3, s)
        ctx.ring_l2sq_device(d_x.data_ptr(), count, width, d_l2.data_ptr(), s)
    for replay in range(2):
        x = _short(rng, q, bound, (count, width, n))
        if replay == 1:
            x[1, 2, 5] = bound + 1                                # a replay also redoes the status and the clearing
        d_x.copy_(_dev(torch, x))
        graph.replay()
        torch.cuda.synchronize()
        eager, eager_status = ctx.ring_project(x, bound, keys, components=2, index_base=3)
        assert eager_status.tolist() == ([1, 1, 1] if replay == 0 else [1, 0, 1])
        assert np.array_equal(d_out.cpu().numpy(), eager) and d_status.cpu().tolist() == eager_status.tolist()
        assert d_l2.cpu().numpy().view(np.uint64).tolist() == _l2_words(ctx.ring_l2sq(x).tolist())
        if replay == 0:
            want, _ = model.project(oracle, q, x, bound, keys.tolist(), 2, 17, 3)
            assert np.array_equal(eager, want)
    ctx.close()
