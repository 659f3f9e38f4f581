"""GPU suite: the batched ring inner product c_j = sum_i a_{j,i} b_{j,i}, lsr_ntt_ring_dot_batch(_device).  Pinned against schoolbook
convolutions (independent of the oracle), against the ring multiply (terms == 1 word for word; identical terms = a multiple of one
product, which drives the accumulator as far as it can go), and against the oracle's composition INTT(sum_i NTT(a_i) . NTT(b_i)) at
every degree 2^1 .. 2^17 in each arithmetic flavour."""
import os
import subprocess
import sys

import numpy as np
import pytest

from ring_tile_model import schoolbook_dot as _schoolbook_dot

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q44 = 17592180539393           # 44-bit prime, 2^18 | q - 1: every n up to 2^17 (FP64 kernels)
Q_NORTH = 17592169062401       # north_star's prime (n <= 4096)
Q16 = 17592182243329           # the n = 2^16 commitment prime
Q60 = 1152921504606584833      # 60-bit prime (u64 Shoup kernels)
GOLD = 18446744069414584321


def _rand(rng, q, shape):
    return rng.integers(0, q, size=shape, dtype=np.uint64)


def _to_u64(values):
    return np.array([int(x) for x in np.ravel(values)], dtype=np.uint64).reshape(np.shape(values))


def _oracle_dot(oracle, q, n, a, b):
    """The oracle's inverse transform of sum_i mul_pointwise(forward a_i, forward b_i), the sum taken mod q in Python integers."""
    batch, terms = a.shape[:2]
    b_full = np.ascontiguousarray(np.broadcast_to(b, a.shape))
    fa = oracle.ntt_forward(q, n, np.ascontiguousarray(a.reshape(-1, n)))
    fb = oracle.ntt_forward(q, n, b_full.reshape(-1, n))
    prod = np.asarray(oracle.mul_pointwise(q, n, fa, fb)).reshape(batch, terms, n).astype(object)
    return oracle.ntt_inverse(q, n, _to_u64(prod.sum(axis=1) % q))


def _dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


# ---- 1. schoolbook ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [12289, Q_NORTH])
@pytest.mark.parametrize("n", [2, 16, 256])
@pytest.mark.parametrize("terms", [1, 2, 5])
def test_matches_schoolbook(pkg, q, n, terms):
    rng = np.random.default_rng(n + terms + q % 1000)
    ctx = pkg.NttContext(q, n, device=0)
    a, b = _rand(rng, q, (3, terms, n)), _rand(rng, q, (3, terms, n))
    assert ctx.ring_dot(a, b).tolist() == _schoolbook_dot(a, b, q, -1), (q, n, terms)
    assert ctx.ring_dot(a, b[1]).tolist() == _schoolbook_dot(a, b[1], q, -1), (q, n, terms, "shared b")
    ctx.close()


def test_cyclic_goldilocks_matches_plain_convolution(pkg):
    n, terms = 16, 3
    rng = np.random.default_rng(16)
    ntt = pkg.CyclicNtt(n)
    a, b = _rand(rng, GOLD, (3, terms, n)), _rand(rng, GOLD, (3, terms, n))
    assert ntt.ring_dot(a, b).tolist() == _schoolbook_dot(a, b, GOLD, 1)
    assert ntt.ring_dot(a, b[2]).tolist() == _schoolbook_dot(a, b[2], GOLD, 1)
    ntt.close()


# ---- 2. terms == 1 is the ring multiply --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [256, 4096, 65536])
def test_one_term_equals_the_ring_multiply(pkg, n):
    q, batch = Q44, 5
    rng = np.random.default_rng(n)
    ctx = pkg.NttContext(q, n, device=0)
    a, b = _rand(rng, q, (batch, n)), _rand(rng, q, (batch, n))
    assert np.array_equal(ctx.ring_dot(a.reshape(batch, 1, n), b.reshape(batch, 1, n)), ctx.ring_mul(a, b)), n
    assert np.array_equal(ctx.ring_dot(a.reshape(batch, 1, n), b[:1]), ctx.ring_mul(a, b[0])), (n, "shared b")
    ctx.close()


# ---- 3. the oracle's composition at every degree, in every flavour ---------------------------------------------------------------
def _batch_for(logn):
    return {8: 7, 16: 3, 17: 2}.get(logn, 5 if logn <= 12 else 2)


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


@pytest.mark.parametrize("flavour", ["f64", "u64_q60", "u64_q44"])
@pytest.mark.parametrize("logn", range(1, 18))
def test_matches_oracle_composition(pkg, oracle, lib, flavour, logn):
    n, terms, batch = 1 << logn, 3, _batch_for(logn)
    q, ctx = _flavour_context(pkg, lib, flavour, n)
    rng = np.random.default_rng(1000 * logn + len(flavour))
    a, b = _rand(rng, q, (batch, terms, n)), _rand(rng, q, (batch, terms, n))
    assert np.array_equal(ctx.ring_dot(a, b), _oracle_dot(oracle, q, n, a, b)), (flavour, n)
    assert np.array_equal(ctx.ring_dot(a, b[0]), _oracle_dot(oracle, q, n, a, b[0])), (flavour, n, "shared b")
    ctx.close()


# ---- 4. the accumulator: identical terms, every product of one sign per residue ----------------------------------------------------
def _identical_terms_case(ctx, q, n, batch, terms, seed):
    """All terms of output j are (a_j, b_j): the sum is terms * (a_j b_j), and the accumulator grows linearly at every residue."""
    rng = np.random.default_rng(seed)
    a, b = _rand(rng, q, (batch, n)), _rand(rng, q, (batch, n))
    one = ctx.ring_mul(a, b).astype(object)
    want = _to_u64(one * (terms % q) % q)
    a_all = np.ascontiguousarray(np.broadcast_to(a[:, None, :], (batch, terms, n)))
    b_all = np.ascontiguousarray(np.broadcast_to(b[:, None, :], (batch, terms, n)))
    assert np.array_equal(ctx.ring_dot(a_all, b_all), want), (terms, "per-output b")
    # one shared vector b (b_0 in every term): output j is terms * (a_j b_0)
    want0 = _to_u64(ctx.ring_mul(a, b[0]).astype(object) * (terms % q) % q)
    assert np.array_equal(ctx.ring_dot(a_all, b_all[0]), want0), (terms, "shared b")


def _recentring_terms(pkg):
    period = pkg.RING_DOT_F64_RECENTRE_PERIOD
    return [2, period, period + 1, 2 * period + 1, 3001]


@pytest.mark.parametrize("which", range(5))
def test_f64_accumulator_is_recentred(pkg, which):
    """n = 1024: four outputs per tile, operand tiles strided by terms * n.  3001 is odd and 3001 q / 2 > 2^54: a sum kept in a double
    without reduction cannot be exact.  All 3001 terms reach ONE launch: host_staged_dot stages 256 MiB / 8 n = 32768 polynomials per
    operand, so the four outputs go up whole, and ring_dot_enqueue hands a per-output b over in one launch and a shared b in groups of
    ring_dot_chunk_polys = 4096 b-hat rows.  (Which positions can tell a lost periodic re-centre: tests/test_f64_long_sums_gpu.py.)"""
    terms = _recentring_terms(pkg)[which]
    assert which != 4 or terms * Q_NORTH // 2 > 2**54
    ctx = pkg.NttContext(Q_NORTH, 1024, device=0)
    assert ctx.uses_f64
    _identical_terms_case(ctx, Q_NORTH, 1024, 4, terms, which)
    ctx.close()


def test_u64_accumulator_is_reduced(pkg):
    ctx = pkg.NttContext(Q60, 1024, device=0)
    assert not ctx.uses_f64
    _identical_terms_case(ctx, Q60, 1024, 4, 41, 60)      # 41 canonical 60-bit summands overflow 64 bits unless each sum is reduced
    ctx.close()


def test_goldilocks_accumulator_is_reduced(pkg):
    ntt = pkg.CyclicNtt(1024)
    _identical_terms_case(ntt, GOLD, 1024, 4, 41, 64)
    ntt.close()


# ---- 5. n = 4096 and n = 2^16; chunked batch and terms ---------------------------------------------------------------------------
@pytest.mark.parametrize("q,n", [(Q_NORTH, 4096), (Q16, 65536)])
@pytest.mark.parametrize("terms", [2, 4])
def test_tile_and_two_pass_sizes(pkg, oracle, q, n, terms):
    rng = np.random.default_rng(n + terms)
    ctx = pkg.NttContext(q, n, device=0)
    a, b = _rand(rng, q, (3, terms, n)), _rand(rng, q, (3, terms, n))
    assert np.array_equal(ctx.ring_dot(a, b), _oracle_dot(oracle, q, n, a, b)), (n, terms)
    assert np.array_equal(ctx.ring_dot(a, b[2]), _oracle_dot(oracle, q, n, a, b[2])), (n, terms, "shared b")
    ctx.close()


_CHUNKED = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as entry
pkg = entry.load_package()
data = np.load(sys.argv[2] + "/in.npz")
ctx = pkg.NttContext(int(data["q"]), 65536, device=0)
np.savez(sys.argv[2] + "/out.npz", each=ctx.ring_dot(data["a"], data["b"]), shared=ctx.ring_dot(data["a"], data["b"][1]))
ctx.close()
"""


def test_chunked_batch_and_terms_equal_the_unchunked_result(pkg, tmp_path):
    """n = 2^16, batch 3, terms 4 under LAMBDA_SNARK_NTT_CHUNK_MIB=3 (read once per process: a fresh child): a third of 3 MiB holds 2
    polynomials per workspace array, so the 4 terms take two passes and every output is a chunk of its own."""
    q, n = Q16, 65536
    rng = np.random.default_rng(53)
    a, b = _rand(rng, q, (3, 4, n)), _rand(rng, q, (3, 4, n))
    ctx = pkg.NttContext(q, n, device=0)
    each, shared = ctx.ring_dot(a, b), ctx.ring_dot(a, b[1])
    ctx.close()
    np.savez(str(tmp_path / "in.npz"), q=np.uint64(q), a=a, b=b)
    script = tmp_path / "chunked.py"
    script.write_text(_CHUNKED)
    subprocess.run([sys.executable, str(script), ROOT, str(tmp_path)], check=True, env=dict(os.environ, LAMBDA_SNARK_NTT_CHUNK_MIB="3"), timeout=300)
    out = np.load(str(tmp_path / "out.npz"))
    assert np.array_equal(out["each"], each)
    assert np.array_equal(out["shared"], shared)


# ---- 6. shared b equals b repeated per output, on device buffers ------------------------------------------------------------------
@pytest.mark.parametrize("q,n", [(Q_NORTH, 4096), (Q16, 65536)])
def test_shared_b_equals_repeated_rows(pkg, q, n):
    import torch
    rng = np.random.default_rng(n)
    batch, terms = 5, 3
    ctx = pkg.NttContext(q, n, device=0)
    a, b = _rand(rng, q, (batch, terms, n)), _rand(rng, q, (terms, n))
    d_a, d_b1, d_bn = _dev(torch, a), _dev(torch, b), _dev(torch, np.broadcast_to(b, (batch, terms, n)))
    c1 = torch.empty((batch, n), dtype=torch.int64, device="cuda")
    cn = torch.empty_like(c1)
    ctx.ring_dot_device(c1.data_ptr(), d_a.data_ptr(), d_b1.data_ptr(), batch, terms, 1, _stream(torch))
    ctx.ring_dot_device(cn.data_ptr(), d_a.data_ptr(), d_bn.data_ptr(), batch, terms, batch, _stream(torch))
    torch.cuda.synchronize()
    assert torch.equal(c1, cn)
    ctx.close()


# ---- 7. ordering and capture ----------------------------------------------------------------------------------------------------
def test_calls_are_ordered_across_streams(pkg, oracle):
    import torch
    q, n, terms = Q16, 65536, 2
    rng = np.random.default_rng(71)
    ctx = pkg.NttContext(q, n, device=0)
    a, b = _rand(rng, q, (4, terms, n)), _rand(rng, q, (4, terms, n))
    b2 = _rand(rng, q, (2, terms, n))
    d_a, d_b, d_b2 = _dev(torch, a), _dev(torch, b), _dev(torch, b2)
    mid = torch.empty((4, n), dtype=torch.int64, device="cuda")       # the first call's c = the second call's a, [2][2][n]
    out = torch.empty((2, n), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ctx.ring_dot_device(mid.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), 4, terms, 4, s1.cuda_stream)
    ctx.ring_dot_device(out.data_ptr(), mid.data_ptr(), d_b2.data_ptr(), 2, terms, 2, s2.cuda_stream)   # no synchronisation between them
    s2.synchronize()
    s1.synchronize()
    want_mid = _oracle_dot(oracle, q, n, a, b)
    assert np.array_equal(_host(mid), want_mid)
    assert np.array_equal(_host(out), _oracle_dot(oracle, q, n, want_mid.reshape(2, terms, n), b2))
    ctx.close()


def test_graph_capture_after_eager_warm_up(pkg):
    import torch
    q, n, batch, terms = Q16, 65536, 2, 2
    rng = np.random.default_rng(72)
    ctx = pkg.NttContext(q, n, device=0)
    d_a = torch.zeros((batch, terms, n), dtype=torch.int64, device="cuda")
    d_b = torch.zeros_like(d_a)
    d_c = torch.empty((batch, n), dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):      # eager warm-up: allocates the workspace
        ctx.ring_dot_device(d_c.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), batch, terms, batch, side.cuda_stream)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ctx.ring_dot_device(d_c.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), batch, terms, batch, _stream(torch))
    for _ in range(2):                 # two replays, each on fresh inputs
        a, b = _rand(rng, q, (batch, terms, n)), _rand(rng, q, (batch, terms, n))
        d_a.copy_(_dev(torch, a))
        d_b.copy_(_dev(torch, b))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_host(d_c), ctx.ring_dot(a, b))
    ctx.close()


def test_first_workspace_call_under_capture_is_refused(pkg):
    import torch
    q, n = Q16, 65536
    ctx = pkg.NttContext(q, n, device=0)
    d = torch.zeros((2, n), dtype=torch.int64, device="cuda")
    e = torch.zeros((2, n), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    rc = None
    with torch.cuda.graph(graph, stream=side):
        d.add_(0)                      # (keeps the captured graph non-empty)
        rc = ctx._lib.lsr_ntt_ring_dot_batch_device(ctx.handle, e.data_ptr(), d.data_ptr(), d.data_ptr(), 2, 1, 2, _stream(torch))
    assert rc == -1
    assert "eager" in pkg._abi.last_error()
    graph.replay()                     # the capture stayed usable
    torch.cuda.synchronize()
    ctx.close()


# ---- 8. refusals on a real context ----------------------------------------------------------------------------------------------
def test_output_overlapping_an_operand_is_refused(pkg):
    import torch
    n, batch, terms = 256, 2, 2
    ctx = pkg.NttContext(Q_NORTH, n, device=0)
    buf = torch.zeros((batch * terms + batch, n), dtype=torch.int64, device="cuda")
    other = torch.zeros((batch * terms, n), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    fn = ctx._lib.lsr_ntt_ring_dot_batch_device
    # c straddling the operand's end / c on the operand's first rows / c right behind the operand (allowed)
    for c_row, rc_want in [(batch * terms - 1, -1), (0, -1), (batch * terms, 0)]:
        assert fn(ctx.handle, buf[c_row].data_ptr(), buf.data_ptr(), other.data_ptr(), batch, terms, batch, _stream(torch)) == rc_want, ("a", c_row)
        assert rc_want == 0 or "overlaps a" in pkg._abi.last_error()
        assert fn(ctx.handle, buf[c_row].data_ptr(), other.data_ptr(), buf.data_ptr(), batch, terms, batch, _stream(torch)) == rc_want, ("b", c_row)
        assert rc_want == 0 or "overlaps b" in pkg._abi.last_error()
    # a shared b is [terms][n]: c right behind it is allowed, c on its last row is not
    assert fn(ctx.handle, buf[terms - 1].data_ptr(), other.data_ptr(), buf.data_ptr(), batch, terms, 1, _stream(torch)) == -1
    assert fn(ctx.handle, buf[terms].data_ptr(), other.data_ptr(), buf.data_ptr(), batch, terms, 1, _stream(torch)) == 0
    torch.cuda.synchronize()
    host = np.zeros((batch * terms + batch, n), dtype=np.uint64)
    assert ctx._lib.lsr_ntt_ring_dot_batch(ctx.handle, host[1].ctypes.data, host.ctypes.data, host.ctypes.data, batch, terms, batch) == -1
    ctx.close()


def test_context_above_two_pass_sizes_is_refused(pkg):
    ntt = pkg.CyclicNtt(1 << 18)
    x = np.zeros((2, 1 << 18), dtype=np.uint64)
    with pytest.raises(pkg.CoreError):
        ntt.ring_dot(x, x)
    assert "131072" in pkg._abi.last_error()
    ntt.close()


def test_terms_above_the_cap_are_refused(pkg):
    import torch
    ctx = pkg.NttContext(12289, 2, device=0)
    terms = pkg.RING_DOT_MAX_TERMS + 1
    d = torch.zeros((2, terms, 2), dtype=torch.int64, device="cuda")
    c = torch.zeros((2, 2), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert ctx._lib.lsr_ntt_ring_dot_batch_device(ctx.handle, c.data_ptr(), d.data_ptr(), d.data_ptr(), 2, terms, 2, _stream(torch)) == -1
    assert "LSR_RING_DOT_MAX_TERMS" in pkg._abi.last_error()
    assert ctx._lib.lsr_ntt_ring_dot_batch_device(ctx.handle, c.data_ptr(), d.data_ptr(), d.data_ptr(), 2, terms - 1, 2, _stream(torch)) == 0
    torch.cuda.synchronize()
    assert not c.any()
    ctx.close()


def test_empty_batch_writes_nothing(pkg):
    import torch
    ctx = pkg.NttContext(Q_NORTH, 256, device=0)
    c = torch.full((2, 256), 7, dtype=torch.int64, device="cuda")
    d = torch.ones((2, 3, 256), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert ctx._lib.lsr_ntt_ring_dot_batch_device(ctx.handle, c.data_ptr(), d.data_ptr(), d.data_ptr(), 0, 3, 1, _stream(torch)) == 0
    torch.cuda.synchronize()
    assert bool((c == 7).all())
    ctx.close()
