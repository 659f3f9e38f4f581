"""GPU suite: the Galois automorphisms sigma_g: X -> X^g and the twisted ring inner product c = sum_i sigma_g(a_i) b_i
(lsr_ntt_ring_automorphism_batch / _device, lsr_ntt_ring_dot_galois_batch / _device).  Pinned against the scatter
definition, by the group law and the ring homomorphism in every arithmetic flavour at every kernel form, the fused call word for word
against the composition of the two plain calls, its constant term against the integer inner product, at the accumulator's worst case,
under a shrunken workspace (term groups), in its refusals that read the context, and in its device form across streams and under
graph capture.
Every flavour and tile size LT = 1 .. 12 of both kernels against CPU references: tests/test_ring_galois_fold_sweep_gpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from ring_galois_model import automorphism, automorphism_batch, galois_elements
from test_ring_matvec_gpu import _flavour_context

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q44 = 17592180539393           # 44-bit prime, 2^18 | q - 1: every n up to 2^17 (FP64 kernels)
Q_NORTH = 17592169062401       # north_star's prime (n <= 4096)
Q60 = 1152921504606584833      # 60-bit prime (u64 Shoup kernels)
GOLD = 18446744069414584321
FLAVOURS = ["f64", "u64_q60", "u64_q44"]


def _rand(rng, q, shape):
    return rng.integers(0, q, size=shape, dtype=np.uint64)


def _dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _valid(gs, order):
    """The distinct odd elements of gs below N, in order."""
    return [g for i, g in enumerate(gs) if g % 2 == 1 and 1 <= g < order and g not in gs[:i]]


# ---- 1. the scatter definition ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [12289, Q_NORTH])
@pytest.mark.parametrize("n", [2, 16, 256])
def test_matches_the_model(pkg, q, n):
    rng = np.random.default_rng(n + q % 1000)
    ctx = pkg.NttContext(q, n, device=0)
    assert ctx.galois_conjugation == 2 * n - 1
    gs = galois_elements(n, -1) if n <= 16 else [1, 3, 5, n + 1, 2 * n - 1]
    for count in (1, 3):
        x = _rand(rng, q, (count, n))
        x[0, : min(n, 2)] = [0, q - 1][: min(n, 2)]               # -0 = 0 and -(q - 1) = 1 wherever these words land
        for g in gs:
            assert ctx.ring_automorphism(x, g).tolist() == automorphism_batch(x.tolist(), g, q, -1), (q, n, count, g)
    x = _rand(rng, q, (2, 3, n))                                   # [..., n] keeps its shape; [n] too
    assert ctx.ring_automorphism(x, 3).tolist() == automorphism_batch(x.tolist(), 3, q, -1)
    assert ctx.ring_automorphism(x[0, 0], 3).tolist() == automorphism(x[0, 0].tolist(), 3, q, -1)
    ctx.close()


def test_cyclic_goldilocks_matches_the_model(pkg):
    n = 16
    rng = np.random.default_rng(16)
    ntt = pkg.CyclicNtt(n)
    assert ntt.galois_conjugation == n - 1
    x = _rand(rng, GOLD, (3, n))
    x[0, :2] = [0, GOLD - 1]
    for g in galois_elements(n, 1):
        assert ntt.ring_automorphism(x, g).tolist() == automorphism_batch(x.tolist(), g, GOLD, 1), g
    ntt.close()


# ---- 2. the group law, at every kernel form --------------------------------------------------------------------------------------------
def _group_law(ctx, rng, q, n, order, count):
    x = _rand(rng, q, (count, n))
    assert np.array_equal(ctx.ring_automorphism(x, 1), x)
    far = order - 5                                                # j h passes 2^32 at n >= 2^16: the masked 32-bit product is exact
    gs = _valid([3, 5, n // 2 + 1, order - 1, far, pow(far, -1, order)], order)
    assert n < 1 << 16 or any((n - 1) * pow(g, -1, order) >= 1 << 32 for g in gs)
    for g in gs:
        inv = pow(g, -1, order)
        sx = ctx.ring_automorphism(x, g)
        assert np.array_equal(ctx.ring_automorphism(sx, inv), x), (n, g)
        for h in gs[:3] + [far]:
            assert np.array_equal(ctx.ring_automorphism(sx, h), ctx.ring_automorphism(x, g * h % order)), (n, g, h)


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("n", [256, 4096, 8192, 65536, 131072])
def test_group_law(pkg, lib, flavour, n):
    q, ctx = _flavour_context(pkg, lib, flavour, n)
    _group_law(ctx, np.random.default_rng(n + len(flavour)), q, n, 2 * n, 3)
    ctx.close()


def test_group_law_on_a_large_cyclic_context(pkg):
    n = 1 << 18
    ntt = pkg.CyclicNtt(n)
    _group_law(ntt, np.random.default_rng(18), GOLD, n, n, 1)
    ntt.close()


# ---- 3. the ring homomorphism (catches any sign error) ---------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("n", [256, 4096, 65536])
def test_ring_homomorphism(pkg, lib, flavour, n):
    q, ctx = _flavour_context(pkg, lib, flavour, n)
    rng = np.random.default_rng(3 * n + len(flavour))
    a, b = _rand(rng, q, (2, n)), _rand(rng, q, (2, n))
    ab = ctx.ring_mul(a, b)
    for g in (n + 1, 2 * n - 1, 5):
        assert np.array_equal(ctx.ring_automorphism(ab, g), ctx.ring_mul(ctx.ring_automorphism(a, g), ctx.ring_automorphism(b, g))), (flavour, n, g)
    ctx.close()


# ---- 4. fused equals composed, word for word -------------------------------------------------------------------------------------------
def _fused_equals_composed(ctx, rng, q, n, batch, order, gs):
    for terms in (1, 3):
        a = _rand(rng, q, (batch, terms, n))
        a[0, 0, : min(n, 2)] = [0, q - 1][: min(n, 2)]
        for b_rows in (1, batch):
            b = _rand(rng, q, (terms, n) if b_rows == 1 else (batch, terms, n))
            plain = ctx.ring_dot(a, b)
            for g in _valid(gs, order):
                want = plain if g == 1 else ctx.ring_dot(ctx.ring_automorphism(a, g), b)
                assert np.array_equal(ctx.ring_dot_galois(a, b, g), want), (n, batch, terms, b_rows, g)


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("n,batch", [(2, 3), (256, 19), (2048, 3), (4096, 2)])
def test_fused_equals_composed(pkg, lib, flavour, n, batch):
    """(256, 19): a full tile of 16 outputs and a ragged one of 3; (2048, 3): a tile of 2 outputs and a ragged one of 1."""
    q, ctx = _flavour_context(pkg, lib, flavour, n)
    _fused_equals_composed(ctx, np.random.default_rng(n + batch + len(flavour)), q, n, batch, 2 * n, [1, 5, n + 1, 2 * n - 1])
    ctx.close()


def test_fused_equals_composed_cyclic_goldilocks(pkg):
    n = 256
    ntt = pkg.CyclicNtt(n)
    _fused_equals_composed(ntt, np.random.default_rng(256), GOLD, n, 19, n, [1, 5, n // 2 + 1, n - 1])
    ntt.close()


# ---- 5. the constant term of conj(a) b is the integer inner product --------------------------------------------------------------------
@pytest.mark.parametrize("ring", ["negacyclic", "cyclic"])
def test_constant_term_is_the_inner_product(pkg, ring):
    n, batch, terms = 256, 3, 3
    q = Q_NORTH if ring == "negacyclic" else GOLD
    ctx = pkg.NttContext(q, n, device=0) if ring == "negacyclic" else pkg.CyclicNtt(n)
    rng = np.random.default_rng(5 + len(ring))
    a, b = _rand(rng, q, (batch, terms, n)), _rand(rng, q, (batch, terms, n))
    got = ctx.ring_dot_galois(a, b, ctx.galois_conjugation)
    for j in range(batch):
        want = sum(int(x) * int(y) for x, y in zip(a[j].ravel().tolist(), b[j].ravel().tolist())) % q
        assert int(got[j, 0]) == want, (ring, j)
    ctx.close()


# ---- 6. the accumulator's worst case through the new load ------------------------------------------------------------------------------
def _conjugate_of_minus_ones_times_minus_ones(q, n):
    """sigma_{2n-1}(a) b in X^n + 1 for a = b = -(1 + X + ... + X^(n-1)), from the model's sigma(a): with every b_k = -1, coefficient k
    is -(sum_{i <= k} s_i - sum_{i > k} s_i) over the centred words s of sigma(a) — prefix sums, no kernel involved."""
    s = [w - q if w > q // 2 else w for w in automorphism([q - 1] * n, 2 * n - 1, q, -1)]
    assert s == [-1] + [1] * (n - 1)                               # -1 - sum_k X^-k = -1 + sum_{m >= 1} X^m
    total, prefix, out = sum(s), 0, []
    for k in range(n):
        prefix += s[k]
        out.append(-(prefix - (total - prefix)))
    assert out == [n - 2 * k for k in range(n)]
    return out


def _all_minus_one_case(ctx, q, n, terms):
    a = np.full((2, terms, n), q - 1, dtype=np.uint64)
    one = _conjugate_of_minus_ones_times_minus_ones(q, n)
    want = [[terms * c % q for c in one]] * 2
    for b_shape in [(terms, n), (2, terms, n)]:
        assert ctx.ring_dot_galois(a, np.full(b_shape, q - 1, dtype=np.uint64), 2 * n - 1).tolist() == want, (terms, b_shape)


@pytest.mark.parametrize("terms", [2, 33, 65])
def test_f64_accumulator_worst_case(pkg, terms):
    assert pkg.RING_DOT_F64_RECENTRE_PERIOD == 32
    ctx = pkg.NttContext(Q44, 4096, device=0)
    assert ctx.uses_f64
    _all_minus_one_case(ctx, Q44, 4096, terms)
    ctx.close()


def test_u64_accumulator_worst_case(pkg):
    ctx = pkg.NttContext(Q60, 4096, device=0)
    assert not ctx.uses_f64
    _all_minus_one_case(ctx, Q60, 4096, 33)
    ctx.close()


# ---- 7. term groups under a shrunken workspace -----------------------------------------------------------------------------------------
_CHUNKED = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as entry
pkg = entry.load_package()
data = np.load(sys.argv[2] + "/in.npz")
ctx = pkg.NttContext(int(data["q"]), int(data["n"]), device=0)
a, b, g = data["a"], data["b"], int(data["g"])
fused = ctx.ring_dot_galois(a, b, g)
composed = ctx.ring_dot(ctx.ring_automorphism(a, g), b)
ctx.close()
np.savez(sys.argv[2] + "/out.npz", fused=fused, composed=composed)
"""


def test_term_groups_equal_the_ungrouped_result(pkg, tmp_path):
    """LAMBDA_SNARK_NTT_CHUNK_MIB is read once per process: a fresh child.  Under 6 MiB the workspace holds 64 b-hat rows at
    n = 4096, so 70 terms of a shared b are two launches with the accumulator waiting in c between them."""
    q, n, batch, terms, g = Q44, 4096, 2, 70, 5
    rng = np.random.default_rng(70)
    a, b = _rand(rng, q, (batch, terms, n)), _rand(rng, q, (terms, n))
    ctx = pkg.NttContext(q, n, device=0)
    want = ctx.ring_dot_galois(a, b, g)
    assert np.array_equal(want, ctx.ring_dot(ctx.ring_automorphism(a, g), b))
    ctx.close()
    np.savez(str(tmp_path / "in.npz"), q=np.uint64(q), n=np.uint64(n), g=np.uint64(g), a=a, b=b)
    script = tmp_path / "chunked.py"
    script.write_text(_CHUNKED)
    subprocess.run([sys.executable, str(script), ROOT, str(tmp_path)], check=True, env=dict(os.environ, LAMBDA_SNARK_NTT_CHUNK_MIB="6"), timeout=300)
    out = np.load(str(tmp_path / "out.npz"))
    assert np.array_equal(out["fused"], out["composed"])
    assert np.array_equal(out["fused"], want)


# ---- 8. the refusals that read the context ---------------------------------------------------------------------------------------------
def test_g_outside_the_group_is_refused(pkg):
    n = 256
    for ctx, order in [(pkg.NttContext(Q_NORTH, n, device=0), 2 * n), (pkg.CyclicNtt(n), n)]:
        x = np.zeros((1, n), dtype=np.uint64)
        for g in (order, order + 1, order + 3, (1 << 64) - 1):
            with pytest.raises(pkg.CoreError):
                ctx.ring_automorphism(x, g)
            assert "g = " + str(g) in pkg._abi.last_error()
            with pytest.raises(pkg.CoreError):
                ctx.ring_dot_galois(x[None], x[None], g)
            assert "g = " + str(g) in pkg._abi.last_error()
        assert np.array_equal(ctx.ring_automorphism(x, order - 1), x)      # the largest element is served
        ctx.close()


def test_fused_form_above_4096_is_refused_and_names_the_composition(pkg):
    n = 8192
    ctx = pkg.NttContext(Q44, n, device=0)
    x = np.zeros((1, 1, n), dtype=np.uint64)
    with pytest.raises(pkg.CoreError):
        ctx.ring_dot_galois(x, x, 5)
    msg = pkg._abi.last_error()
    assert "4096" in msg and "lsr_ntt_ring_automorphism_batch_device" in msg and "lsr_ntt_ring_dot_batch_device" in msg
    ctx.close()


def test_output_overlapping_an_operand_is_refused(pkg):
    import torch
    n, batch, terms = 256, 2, 3
    ctx = pkg.NttContext(Q_NORTH, n, device=0)
    buf = torch.zeros((2 * batch * terms, n), dtype=torch.int64, device="cuda")
    other = torch.zeros((batch * terms, n), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.current_stream().cuda_stream
    auto, dot = ctx._lib.lsr_ntt_ring_automorphism_batch_device, ctx._lib.lsr_ntt_ring_dot_galois_batch_device
    # out on x / out straddling x's end / out right behind x (allowed)
    for row, rc_want in [(0, -1), (batch - 1, -1), (batch, 0)]:
        assert auto(ctx.handle, buf[row].data_ptr(), buf.data_ptr(), batch, 3, s) == rc_want, row
        msg = pkg._abi.last_error()
        assert rc_want == 0 or ("out overlaps x" in msg and "lsr_ntt_ring_automorphism_batch_device:" in msg)
    for row, rc_want in [(0, -1), (batch * terms - 1, -1), (batch * terms, 0)]:
        assert dot(ctx.handle, buf[row].data_ptr(), buf.data_ptr(), other.data_ptr(), batch, terms, batch, 3, s) == rc_want, ("a", row)
        msg = pkg._abi.last_error()
        assert rc_want == 0 or ("c overlaps a" in msg and "lsr_ntt_ring_dot_galois_batch_device:" in msg)
        assert dot(ctx.handle, buf[row].data_ptr(), other.data_ptr(), buf.data_ptr(), batch, terms, batch, 3, s) == rc_want, ("b", row)
        msg = pkg._abi.last_error()
        assert rc_want == 0 or ("c overlaps b" in msg and "lsr_ntt_ring_dot_galois_batch_device:" in msg)
    torch.cuda.synchronize()
    host = np.zeros((2 * batch, n), dtype=np.uint64)
    assert ctx._lib.lsr_ntt_ring_automorphism_batch(ctx.handle, host[1].ctypes.data, host.ctypes.data, batch, 3) == -1
    assert "lsr_ntt_ring_automorphism_batch:" in pkg._abi.last_error()
    ctx.close()


# ---- 9. the device form ----------------------------------------------------------------------------------------------------------------
def test_device_form_is_ordered_across_streams(pkg):
    """A ring inner product on one stream writes what the twisted inner product on another stream reads, with no synchronisation
    between them: the context's ring event orders the two."""
    import torch
    q, n, batch, terms, g = Q_NORTH, 4096, 2, 2, 2 * 4096 - 1
    rng = np.random.default_rng(n + 9)
    ctx = pkg.NttContext(q, n, device=0)
    a, b = _rand(rng, q, (batch * terms, 2, n)), _rand(rng, q, (batch * terms, 2, n))
    w = _rand(rng, q, (terms, n))
    d_a, d_b, d_w = _dev(torch, a), _dev(torch, b), _dev(torch, w)
    d_v = torch.empty((batch, terms, n), dtype=torch.int64, device="cuda")
    d_c = torch.empty((batch, n), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ctx.ring_dot_device(d_v.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), batch * terms, 2, batch * terms, s1.cuda_stream)
    ctx.ring_dot_galois_device(d_c.data_ptr(), d_v.data_ptr(), d_w.data_ptr(), batch, terms, 1, g, s2.cuda_stream)
    s2.synchronize()
    s1.synchronize()
    v = ctx.ring_dot(a, b).reshape(batch, terms, n)
    assert np.array_equal(_host(d_v), v)
    assert np.array_equal(_host(d_c), ctx.ring_dot(ctx.ring_automorphism(v, g), w))
    ctx.close()


def test_graph_capture_after_eager_warm_up(pkg):
    """Captured on one stream: y = sigma_g1(x), then c = sum_i sigma_g2(y_i) w_i with a shared w (the form that needs the workspace)."""
    import torch
    q, n, batch, terms, g1, g2 = Q_NORTH, 256, 3, 2, 5, 2 * 256 - 1
    rng = np.random.default_rng(91)
    ctx = pkg.NttContext(q, n, device=0)
    d_x = torch.zeros((batch, terms, n), dtype=torch.int64, device="cuda")
    d_y = torch.zeros_like(d_x)
    d_w = torch.zeros((terms, n), dtype=torch.int64, device="cuda")
    d_c = torch.empty((batch, n), dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):      # eager warm-up: allocates the workspace (the automorphism needs none)
        ctx.ring_dot_galois_device(d_c.data_ptr(), d_y.data_ptr(), d_w.data_ptr(), batch, terms, 1, g2, side.cuda_stream)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        s = torch.cuda.current_stream().cuda_stream
        ctx.ring_automorphism_device(d_y.data_ptr(), d_x.data_ptr(), batch * terms, g1, s)
        ctx.ring_dot_galois_device(d_c.data_ptr(), d_y.data_ptr(), d_w.data_ptr(), batch, terms, 1, g2, s)
    for _ in range(2):                 # two replays, each on fresh inputs
        x, w = _rand(rng, q, (batch, terms, n)), _rand(rng, q, (terms, n))
        d_x.copy_(_dev(torch, x))
        d_w.copy_(_dev(torch, w))
        graph.replay()
        torch.cuda.synchronize()
        assert _host(d_y).tolist() == automorphism_batch(x.tolist(), g1, q, -1)
        assert np.array_equal(_host(d_c), ctx.ring_dot(ctx.ring_automorphism(x, g1 * g2 % (2 * n)), w))
    ctx.close()


def test_first_shared_b_call_under_capture_is_refused(pkg):
    import torch
    q, n, batch, terms, g = Q_NORTH, 64, 3, 2, 3
    rng = np.random.default_rng(92)
    ctx = pkg.NttContext(q, n, device=0)
    a, w = _rand(rng, q, (batch, terms, n)), _rand(rng, q, (terms, n))
    d_a, d_w = _dev(torch, a), _dev(torch, w)
    d_y = torch.zeros((batch, terms, n), dtype=torch.int64, device="cuda")
    d_c = torch.zeros((batch, n), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    rc = None
    with torch.cuda.graph(graph, stream=side):
        s = torch.cuda.current_stream().cuda_stream
        ctx.ring_automorphism_device(d_y.data_ptr(), d_a.data_ptr(), batch * terms, g, s)      # no workspace: capturable with no warm-up
        rc = ctx._lib.lsr_ntt_ring_dot_galois_batch_device(ctx.handle, d_c.data_ptr(), d_a.data_ptr(), d_w.data_ptr(), batch, terms, 1, g, s)
    assert rc == -1
    msg = pkg._abi.last_error()
    assert "workspace" in msg and "eager" in msg
    graph.replay()                     # the capture stayed usable
    torch.cuda.synchronize()
    assert not bool(d_c.any())         # and holds no launch of the refused call
    assert _host(d_y).tolist() == automorphism_batch(a.tolist(), g, q, -1)
    ctx.ring_dot_galois_device(d_c.data_ptr(), d_a.data_ptr(), d_w.data_ptr(), batch, terms, 1, g, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(_host(d_c), ctx.ring_dot(_host(d_y), w))      # the context still works
    ctx.close()
