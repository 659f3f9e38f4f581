"""GPU suite: the fold of ring vectors by ring-valued challenges, out[j][c] = sum_i p[j][i] v[j term_stride + i][c]
(lsr_ntt_ring_fold_batch / _device).  Pinned against the schoolbook definition, word for word against the ring inner
product on the gathered operands in every arithmetic flavour, against the oracle's composition INTT(sum NTT . NTT) at every degree
2^1 .. 2^17, at the accumulator's worst case, under a shrunken workspace (term groups, component chunks), in the commitment chain it
exists for, and in its device form across streams and under graph capture.
Every flavour and tile size against CPU references: tests/test_ring_galois_fold_sweep_gpu.py (LT = 1 .. 12) and
tests/test_ring_cyclic_two_pass_gpu.py (the cyclic MID instantiations)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ring_tile_model as model
from ring_fold_model import gather, schoolbook_fold, vectors_needed
from test_ring_matvec_gpu import _flavour_context

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q44 = 17592180539393           # 44-bit prime, 2^18 | q - 1: every n up to 2^17 (FP64 kernels)
Q_NORTH = 17592169062401       # north_star's prime (n <= 4096)
Q60 = 1152921504606584833      # 60-bit prime (u64 Shoup kernels)
GOLD = 18446744069414584321


def _rand(rng, q, shape):
    return rng.integers(0, q, size=shape, dtype=np.uint64)


def _operands(rng, q, n, outputs, terms, stride, width):
    return _rand(rng, q, (vectors_needed(outputs, terms, stride), width, n)), _rand(rng, q, (outputs, terms, n))


def _dot_route(ctx, v, p, stride):
    """The ring inner product on the gathered operands, reshaped to the fold's output."""
    a, b = gather(v, p, stride)
    return ctx.ring_dot(a, b).reshape(p.shape[0], v.shape[1], v.shape[2])


def _dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


# ---- 1. schoolbook ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [12289, Q_NORTH])
@pytest.mark.parametrize("n", [2, 16, 256])
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 2, 2), (2, 3, 5)])
def test_matches_schoolbook(pkg, q, n, shape):
    outputs, terms, width = shape
    rng = np.random.default_rng(n + 10 * terms + q % 1000)
    ctx = pkg.NttContext(q, n, device=0)
    for stride in (0, terms):
        v, p = _operands(rng, q, n, outputs, terms, stride, width)
        assert ctx.ring_fold(v, p, stride).tolist() == schoolbook_fold(v, p, stride, q, -1), (q, n, shape, stride)
    ctx.close()


def test_cyclic_goldilocks_matches_plain_convolution(pkg):
    n = 16
    rng = np.random.default_rng(16)
    ntt = pkg.CyclicNtt(n)
    for outputs, terms, width in [(1, 1, 1), (3, 2, 2), (2, 3, 5)]:
        for stride in (0, terms):
            v, p = _operands(rng, GOLD, n, outputs, terms, stride, width)
            assert ntt.ring_fold(v, p, stride).tolist() == schoolbook_fold(v, p, stride, GOLD, 1), (outputs, terms, width, stride)
    ntt.close()


# ---- 2. word for word against the ring inner product on the gathered operands ------------------------------------------------------
@pytest.mark.parametrize("flavour", ["f64", "u64_q60", "u64_q44"])
@pytest.mark.parametrize("n,width,outputs", [(256, 19, 3), (4096, 2, 3), (8192, 3, 2), (65536, 3, 2)])
def test_equals_ring_dot_on_gathered_operands(pkg, lib, flavour, n, width, outputs):
    """n = 256, width 19: a full tile of 16 components and a ragged one of 3."""
    terms = 3
    q, ctx = _flavour_context(pkg, lib, flavour, n)
    rng = np.random.default_rng(n + width + len(flavour))
    for stride in (0, 1, terms, terms + 2):
        v, p = _operands(rng, q, n, outputs, terms, stride, width)
        assert np.array_equal(ctx.ring_fold(v, p, stride), _dot_route(ctx, v, p, stride)), (flavour, n, stride)
    ctx.close()


@pytest.mark.parametrize("flavour", ["f64", "u64_q60", "u64_q44"])
@pytest.mark.parametrize("n", [256, 4096, 8192, 65536])
def test_width_one_disjoint_is_the_ring_dot_itself(pkg, lib, flavour, n):
    outputs, terms = 3, 3
    q, ctx = _flavour_context(pkg, lib, flavour, n)
    rng = np.random.default_rng(n + len(flavour))
    a, b = _rand(rng, q, (outputs, terms, n)), _rand(rng, q, (outputs, terms, n))
    got = ctx.ring_fold(a.reshape(outputs * terms, 1, n), b, terms)      # no gather: v is a, vector by vector
    assert np.array_equal(got.reshape(outputs, n), ctx.ring_dot(a, b)), (flavour, n)
    ctx.close()


# ---- 3. the oracle's composition at every degree -----------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", ["f64", "u64_q60"])
@pytest.mark.parametrize("logn", range(1, 18))
def test_matches_oracle_composition(pkg, oracle, lib, flavour, logn):
    n, outputs, terms, width = 1 << logn, 2, 3, 2
    q, ctx = _flavour_context(pkg, lib, flavour, n)
    rng = np.random.default_rng(1000 * logn + len(flavour))
    stride = (0, 1, terms)[logn % 3]
    v, p = _operands(rng, q, n, outputs, terms, stride, width)
    a, b = gather(v, p, stride)
    want = model.oracle_dot(oracle, q, n, a, b, False, 0).reshape(outputs, width, n)
    assert np.array_equal(ctx.ring_fold(v, p, stride), want), (flavour, n, stride)
    ctx.close()


# ---- 4. the accumulator's worst case: every word q - 1 -------------------------------------------------------------------------------
def _all_minus_one_case(ctx, q, n, terms, sign):
    """Every word of v and p is q - 1 = -1: a product is (sum_k X^k)^2, coefficient k of which is 2 k + 2 - n in X^n + 1 and n in
    X^n - 1; every term adds the same value at every residue, so the accumulator grows as far as `terms` can drive it."""
    width = 2
    v = np.full((terms, width, n), q - 1, dtype=np.uint64)
    p = np.full((1, terms, n), q - 1, dtype=np.uint64)
    one = [(2 * k + 2 - n) if sign < 0 else n for k in range(n)]
    want = [[[terms * c % q for c in one]] * width]
    assert ctx.ring_fold(v, p, 0).tolist() == want, terms


@pytest.mark.parametrize("terms", [2, 32, 33, 65, 3001])
def test_f64_accumulator_is_recentred(pkg, terms):
    """32 is the re-centring period (33, 65: one product past it); 3001 (q - 1)^2-sized summands cannot stay exact in a double
    without reduction.  All 3001 terms reach ONE launch: the one output fits the staging bound (256 MiB / 8 n = 131072 polynomials)
    and ring_fold_enqueue takes whole outputs while terms <= ring_dot_chunk_polys = 4096.  (Which positions can tell a lost periodic
    re-centre: tests/test_f64_long_sums_gpu.py.)"""
    assert pkg.RING_DOT_F64_RECENTRE_PERIOD == 32
    ctx = pkg.NttContext(Q44, 256, device=0)
    assert ctx.uses_f64
    _all_minus_one_case(ctx, Q44, 256, terms, -1)
    ctx.close()


def test_u64_accumulator_is_reduced(pkg):
    ctx = pkg.NttContext(Q60, 256, device=0)
    assert not ctx.uses_f64
    _all_minus_one_case(ctx, Q60, 256, 33, -1)       # 33 canonical 60-bit summands overflow 64 bits unless each sum is reduced
    ctx.close()


def test_goldilocks_accumulator_is_reduced(pkg):
    ntt = pkg.CyclicNtt(256)
    _all_minus_one_case(ntt, GOLD, 256, 33, 1)
    ntt.close()


# ---- 5. term groups and component chunks under a shrunken workspace -------------------------------------------------------------------
_CHUNKED = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as entry
from ring_fold_model import gather
pkg = entry.load_package()
data = np.load(sys.argv[2] + "/in.npz")
out = {}
for name, n, stride in [tuple(c) for c in data["cases"].tolist()]:
    n, stride = int(n), int(stride)
    ctx = pkg.NttContext(int(data["q"]), n, device=0)
    v, p = data[name + "_v"], data[name + "_p"]
    out[name + "_fold"] = ctx.ring_fold(v, p, stride)
    a, b = gather(v, p, stride)
    out[name + "_dot"] = ctx.ring_dot(a, b).reshape(out[name + "_fold"].shape)
    ctx.close()
np.savez(sys.argv[2] + "/out.npz", **out)
"""

# (name, n, outputs, terms, width): under LAMBDA_SNARK_NTT_CHUNK_MIB=6 a workspace array holds 64 polynomials at n = 4096 and 4 at 2^16
_CHUNK_SHAPES = [
    ("tile_groups", 4096, 2, 70, 2),       # 70 terms > 64 b-hat rows: two launches per output, the accumulator waits in out
    ("tile_chunks", 4096, 40, 3, 1),       # 21 outputs' challenges per chunk: two chunks of outputs
    ("mid_terms", 65536, 2, 5, 3),         # 4-term groups hold one component: launches term by term, groups of 4 + 1
    ("mid_comps", 65536, 2, 2, 3),         # 2 terms x 3 components > 4: component chunks of 2 + 1
    ("mid_width1", 65536, 2, 6, 1),        # the whole width fits a group: one launch per group of 4 + 2
    ("mid_outputs", 65536, 3, 2, 1),       # whole outputs fit: chunks of 2 + 1 outputs
]


def test_groups_and_chunks_equal_the_unchunked_result(pkg, tmp_path):
    """LAMBDA_SNARK_NTT_CHUNK_MIB is read once per process: a fresh child.  The child's folds are compared with its own ring inner
    products on the gathered operands and with this process's folds under the full workspace."""
    q = Q44
    rng = np.random.default_rng(55)
    arrays, cases, want = {}, [], {}
    for name, n, outputs, terms, width in _CHUNK_SHAPES:
        ctx = pkg.NttContext(q, n, device=0)
        for stride in (0, terms):
            key = f"{name}_{stride}"
            v, p = _operands(rng, q, n, outputs, terms, stride, width)
            arrays[key + "_v"], arrays[key + "_p"] = v, p
            cases.append((key, str(n), str(stride)))
            want[key] = ctx.ring_fold(v, p, stride)
        ctx.close()
    np.savez(str(tmp_path / "in.npz"), q=np.uint64(q), cases=np.array(cases), **arrays)
    script = tmp_path / "chunked.py"
    script.write_text(_CHUNKED)
    subprocess.run([sys.executable, str(script), ROOT, str(tmp_path)], check=True, env=dict(os.environ, LAMBDA_SNARK_NTT_CHUNK_MIB="6"), timeout=300)
    out = np.load(str(tmp_path / "out.npz"))
    for key, _, _ in cases:
        assert np.array_equal(out[key + "_fold"], out[key + "_dot"]), key
        assert np.array_equal(out[key + "_fold"], want[key]), key


# ---- 6. the chain: fold the witnesses, fold the commitments, check M z = y' on the device ---------------------------------------------
def test_folded_witness_opens_the_folded_commitment(pkg):
    import torch
    n, q, rows, cols, outputs, terms, kappa, beta = 256, Q_NORTH, 2, 3, 2, 3, 8, 2
    ctx = pkg.NttContext(q, n, device=0)
    s = torch.cuda.current_stream().cuda_stream
    mat = ctx.ring_matrix_seeded(pkg.ring_sample_key(1), rows, cols)
    keys = torch.from_numpy(np.stack([pkg.ring_sample_key(2), pkg.ring_sample_key(3)]).view(np.int64)).cuda()
    vectors = outputs * terms
    x = torch.empty((vectors, cols, n), dtype=torch.int64, device="cuda")
    p = torch.empty((outputs, terms, n), dtype=torch.int64, device="cuda")
    ctx.ring_sample_device(x.data_ptr(), vectors * cols, pkg.RING_SAMPLE_BOUNDED, beta, keys[0].data_ptr(), vectors * cols, stream=s)
    ctx.ring_sample_device(p.data_ptr(), outputs * terms, pkg.RING_SAMPLE_BALL, kappa, keys[1].data_ptr(), outputs * terms, stream=s)
    z = torch.empty((outputs, cols, n), dtype=torch.int64, device="cuda")
    y = torch.empty((vectors, rows, n), dtype=torch.int64, device="cuda")
    y_fold = torch.empty((outputs, rows, n), dtype=torch.int64, device="cuda")
    mz = torch.empty_like(y_fold)
    linf = torch.empty(outputs * cols, dtype=torch.int64, device="cuda")
    ctx.ring_fold_device(z.data_ptr(), x.data_ptr(), p.data_ptr(), outputs, terms, terms, cols, s)
    mat.matvec_device(y.data_ptr(), x.data_ptr(), vectors, s)
    ctx.ring_fold_device(y_fold.data_ptr(), y.data_ptr(), p.data_ptr(), outputs, terms, terms, rows, s)
    mat.matvec_device(mz.data_ptr(), z.data_ptr(), outputs, s)
    ctx.ring_linf_device(z.data_ptr(), outputs * cols, linf.data_ptr(), s)
    torch.cuda.synchronize()
    assert torch.equal(mz, y_fold)
    assert bool(y_fold.any())
    assert int(_host(linf).max()) <= terms * kappa * beta
    # the challenges are what BALL promises (kappa coefficients +-1) and the fold is the host form's
    ph = _host(p)
    assert ((ph == 1) | (ph == q - 1)).sum(axis=-1).tolist() == [[kappa] * terms] * outputs and int(((ph != 0) & (ph != 1) & (ph != q - 1)).sum()) == 0
    assert np.array_equal(_host(z), ctx.ring_fold(_host(x), ph, terms))
    mat.close()
    ctx.close()


# ---- 7. the device form ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q,n", [(Q_NORTH, 4096), (Q44, 65536)])
def test_device_form_is_ordered_across_streams(pkg, q, n):
    """A ring inner product on one stream writes the vectors the fold on another stream reads, with no synchronisation between them:
    the context's ring event orders the two."""
    import torch
    outputs, terms, width = 2, 2, 2
    rng = np.random.default_rng(n + 7)
    ctx = pkg.NttContext(q, n, device=0)
    vectors = vectors_needed(outputs, terms, terms)
    a, b = _rand(rng, q, (vectors * width, 2, n)), _rand(rng, q, (vectors * width, 2, n))
    p = _rand(rng, q, (outputs, terms, n))
    d_a, d_b, d_p = _dev(torch, a), _dev(torch, b), _dev(torch, p)
    d_v = torch.empty((vectors, width, n), dtype=torch.int64, device="cuda")
    d_out = torch.empty((outputs, width, n), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ctx.ring_dot_device(d_v.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), vectors * width, 2, vectors * width, s1.cuda_stream)
    ctx.ring_fold_device(d_out.data_ptr(), d_v.data_ptr(), d_p.data_ptr(), outputs, terms, terms, width, s2.cuda_stream)
    s2.synchronize()
    s1.synchronize()
    v = ctx.ring_dot(a, b).reshape(vectors, width, n)
    assert np.array_equal(_host(d_v), v)
    assert np.array_equal(_host(d_out), ctx.ring_fold(v, p, terms))
    ctx.close()


def test_graph_capture_after_eager_warm_up(pkg):
    """The fold needs the context's workspace at every n, so n = 64 reaches the path."""
    import torch
    q, n, outputs, terms, width = Q_NORTH, 64, 2, 2, 2
    rng = np.random.default_rng(73)
    ctx = pkg.NttContext(q, n, device=0)
    d_v = torch.zeros((outputs * terms, width, n), dtype=torch.int64, device="cuda")
    d_p = torch.zeros((outputs, terms, n), dtype=torch.int64, device="cuda")
    d_out = torch.empty((outputs, width, n), dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):      # eager warm-up: allocates the workspace
        ctx.ring_fold_device(d_out.data_ptr(), d_v.data_ptr(), d_p.data_ptr(), outputs, terms, terms, width, side.cuda_stream)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ctx.ring_fold_device(d_out.data_ptr(), d_v.data_ptr(), d_p.data_ptr(), outputs, terms, terms, width, torch.cuda.current_stream().cuda_stream)
    for _ in range(2):                 # two replays, each on fresh inputs
        v, p = _operands(rng, q, n, outputs, terms, terms, width)
        d_v.copy_(_dev(torch, v))
        d_p.copy_(_dev(torch, p))
        graph.replay()
        torch.cuda.synchronize()
        assert _host(d_out).tolist() == schoolbook_fold(v, p, terms, q, -1)
    ctx.close()


def test_first_call_under_capture_is_refused(pkg):
    import torch
    q, n, outputs, terms, width = Q_NORTH, 64, 2, 2, 2
    rng = np.random.default_rng(74)
    ctx = pkg.NttContext(q, n, device=0)
    v, p = _operands(rng, q, n, outputs, terms, terms, width)
    d_v, d_p = _dev(torch, v), _dev(torch, p)
    d_out = torch.zeros((outputs, width, n), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    rc = None
    with torch.cuda.graph(graph, stream=side):
        d_out.add_(0)                  # (keeps the captured graph non-empty)
        rc = ctx._lib.lsr_ntt_ring_fold_batch_device(ctx.handle, d_out.data_ptr(), d_v.data_ptr(), d_p.data_ptr(), outputs, terms, terms, width,
                                                     torch.cuda.current_stream().cuda_stream)
    assert rc == -1
    assert "eager" in pkg._abi.last_error()
    graph.replay()                     # the capture stayed usable
    torch.cuda.synchronize()
    assert not bool(d_out.any())       # and holds no launch of the refused call
    ctx.ring_fold_device(d_out.data_ptr(), d_v.data_ptr(), d_p.data_ptr(), outputs, terms, terms, width, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert _host(d_out).tolist() == schoolbook_fold(v, p, terms, q, -1)      # the context still works
    ctx.close()


def test_output_overlapping_an_operand_is_refused(pkg):
    import torch
    n, outputs, terms, width = 256, 2, 2, 3
    ctx = pkg.NttContext(Q_NORTH, n, device=0)
    v_polys, p_polys, out_polys = outputs * terms * width, outputs * terms, outputs * width
    buf = torch.zeros((v_polys + out_polys, n), dtype=torch.int64, device="cuda")
    other = torch.zeros((v_polys, n), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.current_stream().cuda_stream
    fn = ctx._lib.lsr_ntt_ring_fold_batch_device
    # out straddling the operand's end / out on the operand's first rows / out right behind the operand (allowed)
    for row, rc_want in [(v_polys - 1, -1), (0, -1), (v_polys, 0)]:
        assert fn(ctx.handle, buf[row].data_ptr(), buf.data_ptr(), other.data_ptr(), outputs, terms, terms, width, s) == rc_want, ("v", row)
        msg = pkg._abi.last_error()
        assert rc_want == 0 or ("overlaps v" in msg and "lsr_ntt_ring_fold_batch_device" in msg)
    for row, rc_want in [(p_polys - 1, -1), (0, -1), (p_polys, 0)]:
        assert fn(ctx.handle, buf[row].data_ptr(), other.data_ptr(), buf.data_ptr(), outputs, terms, terms, width, s) == rc_want, ("p", row)
        msg = pkg._abi.last_error()
        assert rc_want == 0 or ("overlaps p" in msg and "lsr_ntt_ring_fold_batch_device" in msg)
    torch.cuda.synchronize()
    host = np.zeros((v_polys + out_polys, n), dtype=np.uint64)
    assert ctx._lib.lsr_ntt_ring_fold_batch(ctx.handle, host[1].ctypes.data, host.ctypes.data, host.ctypes.data, outputs, terms, terms, width) == -1
    assert "lsr_ntt_ring_fold_batch:" in pkg._abi.last_error()
    ctx.close()


def test_context_above_two_pass_sizes_is_refused(pkg):
    ntt = pkg.CyclicNtt(1 << 18)
    x = np.zeros((1, 1, 1 << 18), dtype=np.uint64)
    with pytest.raises(pkg.CoreError):
        ntt.ring_fold(x, x, 0)
    assert "131072" in pkg._abi.last_error()
    ntt.close()
