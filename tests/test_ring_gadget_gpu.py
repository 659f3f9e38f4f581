"""GPU suite: gadget decomposition on the device (ring_decompose / ring_recompose / ring_linf and RingMatrix.matvec_gadget with their
_device twins).  Decompose is pinned word for word against the Python-integer model (tests/ring_gadget_model.py); the fused product
y = M G^-1(x) word for word against matvec(decompose(x)) and, at the smallest shapes, against a schoolbook product of the model's
digits.  Every comparison is exact: all of these are integer functions of their inputs.

Two cases the contract names cannot be built and are replaced by what the rules imply:
  * q = 12289 has no context at n = 4096 (2 n must divide q - 1 = 3 * 2^12), so that prime stops at n = 256;
  * no (b, 1) is admissible for any q: B/2 <= floor(q/2) and floor(q/2) <= B^1 - 1 - B/2 = B/2 - 1 contradict each other.  The "D = 1"
    case is therefore a refusal (test_one_digit_is_never_admissible), not a product."""
import numpy as np
import pytest

import ring_gadget_model as model
from ring_gadget_model import GOLDILOCKS, Q14, Q44, Q60, Q_NORTH, UINT64_MAX

pytestmark = pytest.mark.gpu

# kind -> (q, force the u64 kernels, bases to decompose in)
KINDS = {
    "f64_q44": (Q44, False, (2, 4, 11, 32)),
    "f64_north": (Q_NORTH, False, (2, 4, 11, 32)),
    "u64_q44": (Q44, True, (2, 4, 11, 32)),
    "u64_q60": (Q60, False, (4, 16, 32)),
    "f64_q14": (Q14, False, (2, 4, 11)),
}


def _context(pkg, lib, kind, n):
    q, force_u64, bases = KINDS[kind]
    if force_u64:
        lib.lsr_set_arith_mode(1)
    try:
        ctx = pkg.NttContext(q, n, device=0)
    finally:
        lib.lsr_set_arith_mode(0)
    assert ctx.uses_f64 == kind.startswith("f64")
    return q, ctx, bases


def _pairs(q, bases):
    """(b, D) at the minimum D and one above it where that is still admissible (b = 32 has no third digit: 96 > 64)."""
    out = []
    for b in bases:
        d = model.min_digits(q, b)
        assert d >= 2, (q, b)
        out += [(b, dd) for dd in (d, d + 1) if model.admissible(q, b, dd)]
    return out


def _rand(rng, q, shape):
    return rng.integers(0, q, size=shape, dtype=np.uint64)


def _planted(rng, q, count, n):
    """Random elements with the words 0, 1, floor(q/2), floor(q/2) + 1, q - 1 planted at the front of every element (n >= 5), or
    cycling through the elements' positions (n = 2: `count` elements cover all five)."""
    x = _rand(rng, q, (count, n))
    words = [0, 1, q // 2, q // 2 + 1, q - 1]
    for j in range(count):
        for k in range(min(n, 5)):
            x[j, k] = words[(j * min(n, 5) + k) % 5]
    return x


def _dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


# ---- 1. decompose, recompose and the norm against the model --------------------------------------------------------------------
CASES = [(kind, n) for kind in KINDS for n in (2, 16, 256, 4096) if not (kind == "f64_q14" and n == 4096)] + [("f64_q44", 8192)]


@pytest.mark.parametrize("kind,n", CASES)
def test_decompose_equals_the_model_and_recomposes(pkg, lib, kind, n):
    import torch
    q, ctx, bases = _context(pkg, lib, kind, n)
    count = 3 if n <= 256 else 2
    x = _planted(np.random.default_rng(n + len(kind)), q, count, n)
    for b, digits in _pairs(q, bases):
        z = ctx.ring_decompose(x, b, digits)
        assert z.shape == (count, digits, n)
        assert np.array_equal(z, model.decompose(x, q, b, digits)), (kind, n, b, digits)
        assert np.array_equal(ctx.ring_recompose(z, b), x), (kind, n, b, digits, "round trip")
        assert int(ctx.ring_linf(z).max()) <= 1 << (b - 1), (kind, n, b, digits, "digits are short")
    # the device forms, one pair: same words
    b, digits = _pairs(q, bases)[0]
    d_x, d_z, d_back = _dev(torch, x), torch.empty((count, digits, n), dtype=torch.int64, device="cuda"), torch.empty((count, n), dtype=torch.int64, device="cuda")
    ctx.ring_decompose_device(d_z.data_ptr(), d_x.data_ptr(), count, b, digits, _stream(torch))
    ctx.ring_recompose_device(d_back.data_ptr(), d_z.data_ptr(), count, b, digits, _stream(torch))
    torch.cuda.synchronize()
    assert np.array_equal(_host(d_z), model.decompose(x, q, b, digits)) and np.array_equal(_host(d_back), x)
    assert np.array_equal(ctx.ring_decompose(x[0], b, digits), model.decompose(x[0], q, b, digits)), "one element"
    ctx.close()


@pytest.mark.parametrize("kind,n", [("f64_q44", 256), ("u64_q60", 16), ("f64_q14", 2), ("gold", 16)])
def test_recompose_of_arbitrary_residues_equals_the_model(pkg, lib, kind, n):
    """Not short, and shapes only recompose takes: b (D - 1) = 64 with b = 32, D = 3 and with b = 2, D = 33."""
    if kind == "gold":
        q, ctx = GOLDILOCKS, pkg.CyclicNtt(n)
    else:
        q, ctx, _ = _context(pkg, lib, kind, n)
    rng = np.random.default_rng(n)
    for b, digits in [(4, 5), (32, 3), (2, 33), (11, 1)]:
        z = _rand(rng, q, (3, digits, n))
        z[0, :, 0] = q - 1
        assert np.array_equal(ctx.ring_recompose(z, b), model.recompose(z, q, b)), (kind, b, digits)
    ctx.close()


@pytest.mark.parametrize("kind,n", [("f64_q44", 2), ("f64_q44", 256), ("u64_q60", 4096), ("f64_q44", 8192), ("gold", 16)])
def test_linf_on_planted_extremes_and_an_out_of_range_word(pkg, lib, kind, n):
    import torch
    if kind == "gold":
        q, ctx = GOLDILOCKS, pkg.CyclicNtt(n)
    else:
        q, ctx, _ = _context(pkg, lib, kind, n)
    rng = np.random.default_rng(n + 1)
    x = _rand(rng, 1000, (6, n))                          # small words: |centred| < 1000
    x[0, n - 1] = q // 2                                  # the largest positive representative
    x[1, 0] = q // 2 + 1                                  # the most negative one: |.| = q - (q//2 + 1) = floor(q/2), q odd
    x[2, n // 2] = q - 7                                  # -7 among small positive words: the maximum is still below 1000
    x[3, n - 1] = q                                       # not a residue
    x[4, :] = 0
    got = ctx.ring_linf(x)
    assert np.array_equal(got, model.linf(x, q)), (kind, n)
    assert [int(v) for v in got[:2]] == [q // 2, q // 2] and int(got[3]) == UINT64_MAX and int(got[4]) == 0
    assert int(got[2]) < 1000 and int(got[5]) < 1000        # the neighbours of the refused element are unaffected
    d_x, d_l = _dev(torch, x), torch.empty(6, dtype=torch.int64, device="cuda")
    ctx.ring_linf_device(d_x.data_ptr(), 6, d_l.data_ptr(), _stream(torch))
    torch.cuda.synchronize()
    assert np.array_equal(_host(d_l), got)
    ctx.close()


# ---- 2. the fused product ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q,b", [(Q_NORTH, 11), (Q14, 4)])
@pytest.mark.parametrize("n", [2, 16])
@pytest.mark.parametrize("rows,xcols", [(1, 1), (5, 3), (1, 3), (5, 1)])
def test_fused_matches_schoolbook_of_the_models_digits(pkg, q, b, n, rows, xcols):
    digits = model.min_digits(q, b)
    rng = np.random.default_rng(n + 10 * rows + xcols + q % 1000)
    ctx = pkg.NttContext(q, n, device=0)
    m, x = _rand(rng, q, (rows, xcols * digits, n)), _planted(rng, q, 3 * xcols, n).reshape(3, xcols, n)
    mat = ctx.ring_matrix(m)
    y = mat.matvec_gadget(x, b, digits)
    assert np.array_equal(y, mat.matvec(ctx.ring_decompose(x.reshape(-1, n), b, digits).reshape(3, xcols * digits, n)))
    assert np.array_equal(y, model.matvec_schoolbook(m, model.gadget_inverse(x, q, b, digits), q)), (q, n, rows, xcols)
    assert np.array_equal(mat.matvec_gadget(x[1], b, digits), y[1]), "one vector"
    mat.close()
    ctx.close()


@pytest.mark.parametrize("kind,b", [("f64_q44", 16), ("u64_q60", 16), ("u64_q44", 22)])
@pytest.mark.parametrize("n,batch", [(256, 19), (4096, 2)])
def test_fused_equals_matvec_of_the_decomposition(pkg, lib, kind, b, n, batch):
    """n = 256, batch 19: 16 vectors per tile, so the second tile is ragged (3 vectors); rows = row_block + 1: a second, partial row
    block.  Host forms and device forms."""
    import torch
    q, ctx, _ = _context(pkg, lib, kind, n)
    digits, xcols = model.min_digits(q, b), 3
    rng = np.random.default_rng(n + len(kind))
    probe = ctx.ring_matrix(np.zeros((1, 1, n), dtype=np.uint64))
    rows = probe.row_block + 1
    probe.close()
    m, x = _rand(rng, q, (rows, xcols * digits, n)), _planted(rng, q, batch * xcols, n).reshape(batch, xcols, n)
    mat = ctx.ring_matrix(m)
    want = mat.matvec(ctx.ring_decompose(x.reshape(-1, n), b, digits).reshape(batch, xcols * digits, n))
    assert np.array_equal(mat.matvec_gadget(x, b, digits), want), (kind, n)
    d_x, d_y = _dev(torch, x), torch.empty((batch, rows, n), dtype=torch.int64, device="cuda")
    mat.matvec_gadget_device(d_y.data_ptr(), d_x.data_ptr(), batch, b, digits, _stream(torch))
    torch.cuda.synchronize()
    assert np.array_equal(_host(d_y), want), (kind, n, "device form")
    mat.close()
    ctx.close()


@pytest.mark.parametrize("n,batch", [(256, 3), (4096, 1)])
def test_f64_sum_crosses_the_recentring_period(pkg, lib, n, batch):
    """b = 4, D = 12, xcols = 3: 36 matrix columns, so the FP64 accumulator is re-centred after column 31 — in the middle of the third
    x column's digits.  Identical large matrix entries make every product of one residue the same sign."""
    q, ctx, _ = _context(pkg, lib, "f64_north", n)
    b, digits, xcols = 4, 12, 3
    assert model.min_digits(q, b) == digits and xcols * digits > pkg.RING_DOT_F64_RECENTRE_PERIOD
    rng = np.random.default_rng(n)
    m = np.full((2, xcols * digits, n), q - 1, dtype=np.uint64)
    m[1] = _rand(rng, q, (xcols * digits, n))
    x = _planted(rng, q, batch * xcols, n).reshape(batch, xcols, n)
    mat = ctx.ring_matrix(m)
    want = mat.matvec(ctx.ring_decompose(x.reshape(-1, n), b, digits).reshape(batch, xcols * digits, n))
    assert np.array_equal(mat.matvec_gadget(x, b, digits), want)
    mat.close()
    ctx.close()


# ---- 3. refusals that read the context -----------------------------------------------------------------------------------------
def test_one_digit_is_never_admissible(pkg):
    ctx = pkg.NttContext(Q_NORTH, 16, device=0)
    x = np.zeros((1, 16), dtype=np.uint64)
    mat = ctx.ring_matrix(np.zeros((1, 1, 16), dtype=np.uint64))
    for b in (2, 22, 32):
        assert not model.admissible(Q_NORTH, b, 1)
        with pytest.raises(pkg.CoreError, match="not admissible"):
            ctx.ring_decompose(x, b, 1)
        with pytest.raises(pkg.CoreError, match="not admissible"):
            mat.matvec_gadget(x.reshape(1, 1, 16), b, 1)
    mat.close()
    ctx.close()


def test_goldilocks_is_refused_by_the_rule(pkg, lib):
    """No (b, D) with b D <= 64 covers the centred residues of 2^64 - 2^32 + 1: admissibility (checked before cols % digits) refuses."""
    ntt = pkg.CyclicNtt(16)
    mat = ntt.ring_matrix(np.zeros((1, 2, 16), dtype=np.uint64))
    x, y = np.zeros((1, 2, 16), dtype=np.uint64), np.zeros((1, 1, 16), dtype=np.uint64)
    for b, digits in [(32, 2), (16, 4), (2, 32)]:
        assert lib.lsr_ntt_ring_matvec_gadget_batch(mat.handle, y.ctypes.data, x.ctypes.data, 1, b, digits) == -1
        msg = pkg._abi.last_error()
        assert "lsr_ntt_ring_matvec_gadget_batch" in msg and "not admissible" in msg and "gives 0" in msg
        with pytest.raises(pkg.CoreError, match="not admissible"):
            ntt.ring_decompose(x[0, 0], b, digits)
    mat.close()
    ntt.close()


def test_fused_product_above_4096_names_the_calls_to_compose(pkg):
    n, b, digits = 8192, 32, 2
    ctx = pkg.NttContext(Q44, n, device=0)
    mat = ctx.ring_matrix(np.zeros((1, digits, n), dtype=np.uint64))
    with pytest.raises(pkg.CoreError) as err:
        mat.matvec_gadget(np.zeros((1, 1, n), dtype=np.uint64), b, digits)
    msg = str(err.value)
    assert "8192" in msg and "lsr_ntt_ring_decompose_batch_device" in msg and "lsr_ntt_ring_matvec_batch_device" in msg
    mat.close()
    ctx.close()


def test_refusal_order_behind_the_shape_rules(pkg, lib):
    """inadmissible (b, D) -> cols % digits -> the empty call (0) -> overlap, each also when a later rule is broken too."""
    import torch
    n, b = 16, 16
    ctx = pkg.NttContext(Q44, n, device=0)
    mat = ctx.ring_matrix(np.zeros((1, 5, n), dtype=np.uint64))          # 5 columns: no multiple of D = 3
    d = torch.zeros((8, n), dtype=torch.int64, device="cuda")
    p, s = d.data_ptr(), _stream(torch)
    call = lib.lsr_ntt_ring_matvec_gadget_batch_device
    assert model.min_digits(Q44, b) == 3
    for batch in (0, 1):
        assert call(mat.handle, p, p, batch, b, 2, s) == -1 and "not admissible" in pkg._abi.last_error()
        assert call(mat.handle, p, p, batch, b, 3, s) == -1 and "not a multiple" in pkg._abi.last_error()
    mat.close()
    mat = ctx.ring_matrix(np.zeros((1, 6, n), dtype=np.uint64))
    assert call(mat.handle, p, p, 0, b, 3, s) == 0                        # the empty call comes before the overlap check
    assert call(mat.handle, p, p, 1, b, 3, s) == -1 and "overlaps" in pkg._abi.last_error()
    dec = lib.lsr_ntt_ring_decompose_batch_device
    assert dec(ctx.handle, p, p, 0, b, 2, s) == -1 and "not admissible" in pkg._abi.last_error()
    assert dec(ctx.handle, p, p, 0, b, 3, s) == 0
    assert dec(ctx.handle, p, p + 8 * n, 1, b, 3, s) == -1 and "overlaps" in pkg._abi.last_error()
    assert lib.lsr_ntt_ring_recompose_batch_device(ctx.handle, p + 8 * n, p, 1, b, 3, s) == -1 and "overlaps" in pkg._abi.last_error()
    torch.cuda.synchronize()
    mat.close()
    ctx.close()


# ---- 4. graph capture ----------------------------------------------------------------------------------------------------------
def test_device_form_is_capturable_from_the_first_call(pkg):
    """No workspace: the very first call on a fresh context and matrix is the captured one.  Replayed twice, x changed in between."""
    import torch
    q, n, b, batch, rows, xcols = Q_NORTH, 256, 11, 5, 3, 2
    digits = model.min_digits(q, b)
    rng = np.random.default_rng(7)
    ctx = pkg.NttContext(q, n, device=0)
    m = _rand(rng, q, (rows, xcols * digits, n))
    xs = [_rand(rng, q, (batch, xcols, n)) for _ in range(2)]
    mat = ctx.ring_matrix(m)
    d_x, d_y = _dev(torch, xs[0]), torch.zeros((batch, rows, n), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        mat.matvec_gadget_device(d_y.data_ptr(), d_x.data_ptr(), batch, b, digits, torch.cuda.current_stream().cuda_stream)
    for x in xs:
        d_x.copy_(_dev(torch, x))
        graph.replay()
        torch.cuda.synchronize()
        want = model.gadget_inverse(x, q, b, digits)
        assert np.array_equal(_host(d_y), mat.matvec(want))
    mat.close()
    ctx.close()
