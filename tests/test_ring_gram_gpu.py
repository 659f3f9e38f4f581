"""GPU suite: the ring Gram matrices g[j][i][l] = sum_c a[j][i][c] b[j][l][c] (lsr_ntt_ring_gram_batch / _device).
Pinned against the schoolbook definition, word for word against the ring inner product pair by pair in every arithmetic flavour on
every edge of the register block, in where the outputs land, at the accumulators' worst case, under a shrunken workspace (column
groups, family chunks), in the refusals that read the context, and in the device form across streams and under graph capture.
The sweep against models that share nothing with the library, in every flavour, lives in tests/test_ring_gram_sweep_gpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from f64_walk_model import discriminating_positions
from ring_gram_model import dot_pairs, packed_index, pairs, schoolbook_gram
from ring_tile_model import oracle_product
from test_ring_matvec_gpu import _flavour_context

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q44 = 17592180539393           # 44-bit prime, 2^18 | q - 1: every n up to 2^17 (FP64 kernels)
Q_NORTH = 17592169062401       # north_star's prime (n <= 4096)
Q60 = 1152921504606584833      # 60-bit prime (u64 Shoup kernels)
GOLD = 18446744069414584321
SENTINEL = 0x5EA15EA15EA15EA1                 # fits an int64; above every modulus of the tests that fill a buffer with it
MAX_FAMILY_BYTES = 1 << 30


def _rand(rng, q, shape):
    return rng.integers(0, q, size=shape, dtype=np.uint64)


def _dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _dot_route(ctx, a, b):
    """The ring inner product pair by pair, in the order the outputs are stored: [batch][pairs][n]."""
    u, v = dot_pairs(a, b)
    return ctx.ring_dot(u, v).reshape(a.shape[0], -1, a.shape[-1])


def _flat(g):
    return g.reshape(g.shape[0], -1, g.shape[-1])


# ---- 1. schoolbook ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [12289, Q_NORTH])
@pytest.mark.parametrize("n", [2, 16, 256])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 2), (3, 2, 5)])
def test_matches_schoolbook(pkg, q, n, batch, shape):
    ra, rb, width = shape
    rng = np.random.default_rng(n + 10 * ra + 100 * batch + q % 1000)
    ctx = pkg.NttContext(q, n, device=0)
    a, b = _rand(rng, q, (batch, ra, width, n)), _rand(rng, q, (batch, rb, width, n))
    assert ctx.ring_gram(a, b).tolist() == schoolbook_gram(a, b, q, -1), (q, n, batch, shape, "cross")
    assert ctx.ring_gram(a).tolist() == schoolbook_gram(a, None, q, -1), (q, n, batch, shape, "symmetric")
    assert ctx.ring_gram(a[0], b[0]).tolist() == schoolbook_gram(a[:1], b[:1], q, -1)[0]           # 3-d operands: a batch of one
    ctx.close()


def test_cyclic_goldilocks_matches_plain_convolution(pkg):
    n = 16
    rng = np.random.default_rng(16)
    ntt = pkg.CyclicNtt(n)
    for batch in (1, 3):
        for ra, rb, width in [(1, 1, 1), (2, 3, 2), (3, 2, 5)]:
            a, b = _rand(rng, GOLD, (batch, ra, width, n)), _rand(rng, GOLD, (batch, rb, width, n))
            assert ntt.ring_gram(a, b).tolist() == schoolbook_gram(a, b, GOLD, 1), (batch, ra, rb, width)
            assert ntt.ring_gram(a).tolist() == schoolbook_gram(a, None, GOLD, 1), (batch, ra, width)
    ntt.close()


# ---- 2. the edges of the register block, word for word against the ring inner product pair by pair ------------------------------------
@pytest.mark.parametrize("flavour", ["f64", "u64_q60", "u64_q44"])
@pytest.mark.parametrize("n", [256, 4096, 8192, 65536])
@pytest.mark.parametrize("form", ["cross", "symmetric"])
def test_block_edges_equal_ring_dot_per_pair(pkg, lib, flavour, n, form):
    """E = ring_gram_block: a lone vector against a block and a row, one full block, two blocks and a partial one each way; symmetric:
    below one block, one diagonal block, a diagonal and an off-diagonal block with partial blocks of each kind (r = E + 1, 2 E + 1)."""
    batch, width = 2, 3
    q, ctx = _flavour_context(pkg, lib, flavour, n)
    e = ctx.ring_gram_block
    assert e >= 2
    rng = np.random.default_rng(n + len(flavour) + len(form))
    big = n < 8192 or flavour == "f64"                         # 2 E + 1 at n >= 8192: one flavour
    if form == "cross":
        for ra, rb in [(1, e + 1), (e + 1, 1), (e, e)] + ([(2 * e + 1, e + 1)] if big else []):
            a, b = _rand(rng, q, (batch, ra, width, n)), _rand(rng, q, (batch, rb, width, n))
            assert np.array_equal(_flat(ctx.ring_gram(a, b)), _dot_route(ctx, a, b)), (flavour, n, ra, rb)
    else:
        for r in [1, e, e + 1] + ([2 * e + 1] if big else []):
            a = _rand(rng, q, (batch, r, width, n))
            assert np.array_equal(ctx.ring_gram(a), _dot_route(ctx, a, None)), (flavour, n, r)
    ctx.close()


def test_largest_two_pass_degree(pkg):
    n, q = 1 << 17, Q44
    rng = np.random.default_rng(17)
    ctx = pkg.NttContext(q, n, device=0)
    a = _rand(rng, q, (1, 2, 1, n))
    assert np.array_equal(ctx.ring_gram(a), _dot_route(ctx, a, None))
    ctx.close()


# ---- 3. where the outputs land ---------------------------------------------------------------------------------------------------------
def test_symmetric_form_writes_the_packed_triangle_and_nothing_behind_it(pkg):
    import torch
    n, q, batch, width = 256, Q_NORTH, 2, 2
    ctx = pkg.NttContext(q, n, device=0)
    r = ctx.ring_gram_block + 1
    outs = r * (r + 1) // 2
    rng = np.random.default_rng(31)
    a = _rand(rng, q, (batch, r, width, n))
    d_a = _dev(torch, a)
    d_sym = torch.full((batch * outs + 1, n), SENTINEL, dtype=torch.int64, device="cuda")        # one polynomial more than the call owns
    d_full = torch.full((batch * r * r + 1, n), SENTINEL, dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    ctx.ring_gram_device(d_sym.data_ptr(), d_a.data_ptr(), None, batch, r, r, width, s)
    ctx.ring_gram_device(d_full.data_ptr(), d_a.data_ptr(), d_a.data_ptr(), batch, r, r, width, s)     # b = a, the same pointer
    torch.cuda.synchronize()
    sym, full = _host(d_sym), _host(d_full)
    sentinel = np.uint64(SENTINEL)
    assert (sym[-1] == sentinel).all() and (full[-1] == sentinel).all()
    assert (sym[:-1] < q).all() and (full[:-1] < q).all()                # every owned word was written (the sentinel is above q)
    sym, full = sym[:-1].reshape(batch, outs, n), full[:-1].reshape(batch, r, r, n)
    for i, l in pairs(r, r, True):
        assert np.array_equal(sym[:, packed_index(r, i, l)], full[:, i, l]), (i, l)
        assert np.array_equal(full[:, i, l], full[:, l, i]), (i, l)
        assert pkg.ring_gram_index(r, i, l) == packed_index(r, i, l)
    assert np.array_equal(sym, _dot_route(ctx, a, None))
    assert np.array_equal(ctx.ring_gram(a, a), full)                      # the host form with b = a
    ctx.close()


# ---- 4. the accumulators at their worst: every column of a vector is the same polynomial -----------------------------------------------
def _to_u64(values):
    return np.array(values.tolist(), dtype=np.uint64).reshape(values.shape)


def _identical_columns_case(ctx, q, n, width, seed):
    """Vector i is p_i in every column: G[i][l] = width * (p_i p_l), and every accumulator grows linearly at every position."""
    rng = np.random.default_rng(seed)
    pa, pb = _rand(rng, q, (2, n)), _rand(rng, q, (2, n))
    a = np.ascontiguousarray(np.broadcast_to(pa[None, :, None, :], (1, 2, width, n)))
    b = np.ascontiguousarray(np.broadcast_to(pb[None, :, None, :], (1, 2, width, n)))
    scale = lambda x, y: _to_u64(ctx.ring_mul(x, y).astype(object) * (width % q) % q)       # noqa: E731
    want = np.stack([np.stack([scale(pa[i], pb[l]) for l in range(2)]) for i in range(2)])[None]
    assert np.array_equal(ctx.ring_gram(a, b), want), (width, "cross")
    want_sym = np.stack([scale(pa[i], pa[l]) for i, l in pairs(2, 2, True)])[None]
    assert np.array_equal(ctx.ring_gram(a), want_sym), (width, "symmetric")


def _cross_pair_at_launch_capacity(ctx, oracle, q, n, seed):
    """The cross form of ONE vector against one, over as many identical columns as the cross form ever gives one launch: the
    workspace holds 4096 polynomials at every n <= 4096 (gram_workspace_polys) and a launch takes polys / (ra + rb) columns of a
    family, 2048 at ra = rb = 1.  Before the call the walk model is asked which evaluation positions lose a bit over 2048 unreduced
    additions under every representative of the product: without one the call could not tell a lost periodic re-centre."""
    width = 4096 // 2
    rng = np.random.default_rng(seed)
    pa, pb = _rand(rng, q, (1, n)), _rand(rng, q, (1, n))
    fa, fb = (np.array(oracle.ntt_forward(q, n, p).tolist(), dtype=object) for p in (pa, pb))
    telling = len(discriminating_positions(fa * fb % q, q, width))
    assert telling >= 1, "no position of %d can tell a lost re-centre over %d columns" % (n, width)
    a = np.ascontiguousarray(np.broadcast_to(pa[None, :, None, :], (1, 1, width, n)))
    b = np.ascontiguousarray(np.broadcast_to(pb[None, :, None, :], (1, 1, width, n)))
    want = _to_u64(oracle_product(oracle, q, n, pa, pb, False, 0).astype(object) * width % q).reshape(1, 1, 1, n)
    assert np.array_equal(ctx.ring_gram(a, b), want), (width, "cross, one pair", telling)


def test_f64_accumulators_are_recentred_over_3001_columns(pkg, oracle):
    """3001 q / 2 > 2^54: a sum kept in a double without reduction cannot be exact.  (2 + 2) * 3001 polynomials are more than the
    workspace holds at n = 1024, so the sums are also carried between column groups: the cross form of two vectors against two runs
    as launches of 4096 / 4 = 1024 columns with canonical words handed over, and 1024 * 0.875 q < 2^54 additions cannot lose a bit
    that both representatives lose (tests/f64_walk_model.py) — those launches check the hand-over, not the periodic re-centre.  The
    symmetric form of two vectors gets 2048 columns into its first launch, and so does the cross form of one vector against one, which
    _cross_pair_at_launch_capacity adds with the positions that can tell counted first."""
    assert 3001 * Q_NORTH // 2 > 2**54
    ctx = pkg.NttContext(Q_NORTH, 1024, device=0)
    assert ctx.uses_f64
    _identical_columns_case(ctx, Q_NORTH, 1024, 3001, 1)
    _cross_pair_at_launch_capacity(ctx, oracle, Q_NORTH, 1024, 2)
    ctx.close()


def test_u64_accumulators_are_reduced(pkg):
    ctx = pkg.NttContext(Q60, 1024, device=0)
    assert not ctx.uses_f64
    _identical_columns_case(ctx, Q60, 1024, 41, 60)      # 41 canonical 60-bit summands overflow 64 bits unless each sum is reduced
    ctx.close()


def test_goldilocks_accumulators_are_reduced(pkg):
    ntt = pkg.CyclicNtt(1024)
    _identical_columns_case(ntt, GOLD, 1024, 41, 64)
    ntt.close()


@pytest.mark.parametrize("width", [31, 32, 33, 65])
def test_f64_recentring_period_on_both_sides(pkg, width):
    assert pkg.RING_DOT_F64_RECENTRE_PERIOD == 32
    n, q = 256, Q_NORTH
    rng = np.random.default_rng(width)
    ctx = pkg.NttContext(q, n, device=0)
    assert ctx.uses_f64
    a, b = _rand(rng, q, (2, 2, width, n)), _rand(rng, q, (2, 3, width, n))
    assert np.array_equal(_flat(ctx.ring_gram(a, b)), _dot_route(ctx, a, b)), width
    assert np.array_equal(ctx.ring_gram(b), _dot_route(ctx, b, None)), width
    ctx.close()


# ---- 5. column groups and family chunks under a shrunken workspace ---------------------------------------------------------------------
_CHUNKED = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as entry
from ring_gram_model import dot_pairs
pkg = entry.load_package()
data = np.load(sys.argv[2] + "/in.npz")
q = int(data["q"])
out = {}
for name, n, symmetric in [tuple(c) for c in data["cases"].tolist()]:
    ctx = pkg.NttContext(q, int(n), device=0)
    a = data[name + "_a"]
    b = None if symmetric == "1" else data[name + "_b"]
    got = ctx.ring_gram(a, b)
    out[name + "_gram"] = got.reshape(a.shape[0], -1, a.shape[-1])
    u, v = dot_pairs(a, b)
    out[name + "_dot"] = ctx.ring_dot(u, v).reshape(out[name + "_gram"].shape)
    ctx.close()
# 5 + 4 vectors against the 8 polynomials of the workspace at n = 65536: refused, and nothing is written
n = 65536
ctx = pkg.NttContext(q, n, device=0)
a, b = np.zeros((1, 5, 1, n), dtype=np.uint64), np.zeros((1, 4, 1, n), dtype=np.uint64)
g = np.full((1, 5, 4, n), 7, dtype=np.uint64)
rc = ctx._lib.lsr_ntt_ring_gram_batch(ctx.handle, g.ctypes.data, a.ctypes.data, b.ctypes.data, 1, 5, 4, 1)
out["refused_rc"] = np.int64(rc)
out["refused_message"] = np.array(pkg._abi.last_error())
out["refused_untouched"] = np.bool_((g == 7).all())
ctx.close()
np.savez(sys.argv[2] + "/out.npz", **out)
"""

# (name, n, batch, ra, rb (0: symmetric), width): under LAMBDA_SNARK_NTT_CHUNK_MIB=6 the workspace holds 64 polynomials at n = 4096 and 8 at 2^16
_CHUNK_SHAPES = [
    ("cross_groups", 4096, 2, 3, 2, 14),       # (3 + 2) * 14 = 70 > 64: groups of 12 + 2 columns
    ("family_chunks", 4096, 7, 2, 2, 5),       # 20 polynomials per family: chunks of 3 + 3 + 1 families
    ("symmetric_groups", 65536, 2, 3, 0, 5),   # 3 * 5 = 15 > 8: groups of 2 + 2 + 1 columns
]


def test_groups_and_chunks_equal_the_unchunked_result(pkg, tmp_path):
    """LAMBDA_SNARK_NTT_CHUNK_MIB is read once per process: a fresh child.  The child's Gram matrices are compared with its own ring
    inner products pair by pair and with this process's result under the full workspace."""
    q = Q44
    rng = np.random.default_rng(55)
    arrays, cases, want = {}, [], {}
    for name, n, batch, ra, rb, width in _CHUNK_SHAPES:
        ctx = pkg.NttContext(q, n, device=0)
        a = _rand(rng, q, (batch, ra, width, n))
        b = _rand(rng, q, (batch, rb, width, n)) if rb else None
        arrays[name + "_a"] = a
        if rb:
            arrays[name + "_b"] = b
        cases.append((name, str(n), "0" if rb else "1"))
        want[name] = _flat(ctx.ring_gram(a, b))
        ctx.close()
    np.savez(str(tmp_path / "in.npz"), q=np.uint64(q), cases=np.array(cases), **arrays)
    script = tmp_path / "chunked.py"
    script.write_text(_CHUNKED)
    subprocess.run([sys.executable, str(script), ROOT, str(tmp_path)], check=True, env=dict(os.environ, LAMBDA_SNARK_NTT_CHUNK_MIB="6"), timeout=300)
    out = np.load(str(tmp_path / "out.npz"))
    for name, _, _ in cases:
        assert np.array_equal(out[name + "_gram"], out[name + "_dot"]), name
        assert np.array_equal(out[name + "_gram"], want[name]), name
    assert int(out["refused_rc"]) == -1
    assert "LAMBDA_SNARK_NTT_CHUNK_MIB" in str(out["refused_message"]) and "lsr_ntt_ring_gram_batch:" in str(out["refused_message"])
    assert bool(out["refused_untouched"])


# ---- 6. the refusals that read the context ---------------------------------------------------------------------------------------------
def test_output_overlapping_an_operand_is_refused(pkg):
    import torch
    n, batch, ra, rb, width = 256, 2, 2, 3, 2
    ctx = pkg.NttContext(Q_NORTH, n, device=0)
    a_polys, b_polys, g_polys = batch * ra * width, batch * rb * width, batch * ra * rb
    buf = torch.zeros((max(a_polys, b_polys) + g_polys, n), dtype=torch.int64, device="cuda")
    other = torch.zeros((max(a_polys, b_polys), n), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.current_stream().cuda_stream
    fn = ctx._lib.lsr_ntt_ring_gram_batch_device
    # g straddling the operand's end / g on the operand's first rows / g right behind the operand (allowed)
    for row, rc_want in [(a_polys - 1, -1), (0, -1), (a_polys, 0)]:
        assert fn(ctx.handle, buf[row].data_ptr(), buf.data_ptr(), other.data_ptr(), batch, ra, rb, width, s) == rc_want, ("a", row)
        msg = pkg._abi.last_error()
        assert rc_want == 0 or ("overlaps a" in msg and "lsr_ntt_ring_gram_batch_device" in msg)
    for row, rc_want in [(b_polys - 1, -1), (0, -1), (b_polys, 0)]:
        assert fn(ctx.handle, buf[row].data_ptr(), other.data_ptr(), buf.data_ptr(), batch, ra, rb, width, s) == rc_want, ("b", row)
        msg = pkg._abi.last_error()
        assert rc_want == 0 or ("overlaps b" in msg and "lsr_ntt_ring_gram_batch_device" in msg)
    # the symmetric form owns batch * ra (ra + 1) / 2 polynomials
    assert fn(ctx.handle, buf[a_polys - 1].data_ptr(), buf.data_ptr(), None, batch, ra, ra, width, s) == -1
    assert "overlaps a" in pkg._abi.last_error()
    torch.cuda.synchronize()
    host = np.zeros((a_polys + g_polys, n), dtype=np.uint64)
    assert ctx._lib.lsr_ntt_ring_gram_batch(ctx.handle, host[1].ctypes.data, host.ctypes.data, host.ctypes.data, batch, ra, rb, width) == -1
    assert "lsr_ntt_ring_gram_batch:" in pkg._abi.last_error()
    ctx.close()


def test_context_above_two_pass_sizes_is_refused(pkg):
    ntt = pkg.CyclicNtt(1 << 18)
    x = np.zeros((1, 1, 1, 1 << 18), dtype=np.uint64)
    with pytest.raises(pkg.CoreError):
        ntt.ring_gram(x, x)
    assert "131072" in pkg._abi.last_error()
    with pytest.raises(pkg.CoreError):
        ntt.ring_gram(x)
    assert "131072" in pkg._abi.last_error()
    ntt.close()


def test_family_above_the_byte_limit_is_refused_before_any_access(pkg):
    """The buffers handed over hold one polynomial each: the sizes are checked before anything is read or written."""
    import torch
    n = 65536
    ctx = pkg.NttContext(Q44, n, device=0)
    small = torch.full((3, n), SENTINEL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.current_stream().cuda_stream
    fn = ctx._lib.lsr_ntt_ring_gram_batch_device
    g, a, b = (small[k].data_ptr() for k in range(3))
    assert (64 + 64) * 32 * n * 8 > MAX_FAMILY_BYTES and 64 * 64 * n * 8 > MAX_FAMILY_BYTES
    assert 64 * 33 * n * 8 > MAX_FAMILY_BYTES and (32 + 32) * 1 * n * 8 <= MAX_FAMILY_BYTES and 64 * 65 // 2 * n * 8 > MAX_FAMILY_BYTES
    # operands of a cross family; outputs of a cross family (its operands fit); operands and outputs of a symmetric family
    for d_b, ra, rb, width in [(b, 64, 64, 32), (b, 64, 64, 1), (None, 64, 64, 33), (None, 64, 64, 1)]:
        assert fn(ctx.handle, g, a, d_b, 1, ra, rb, width, s) == -1, (ra, rb, width)
        msg = pkg._abi.last_error()
        assert "LSR_RING_GRAM_MAX_FAMILY_BYTES" in msg and "lsr_ntt_ring_gram_batch_device" in msg
    torch.cuda.synchronize()
    assert bool((small == SENTINEL).all())
    ctx.close()


# ---- 7. the device form ------------------------------------------------------------------------------------------------------------
def test_device_form_is_ordered_across_streams(pkg):
    """Two Gram calls on two streams with no synchronisation between them: the first writes the family the second reads, and both
    transform their operands into the one workspace of the context.  The context's ring event orders the two."""
    import torch
    q, n, r, width = Q44, 65536, 2, 3
    rng = np.random.default_rng(n + 7)
    ctx = pkg.NttContext(q, n, device=0)
    a, b = _rand(rng, q, (1, r, width, n)), _rand(rng, q, (1, r, width, n))
    d_a, d_b = _dev(torch, a), _dev(torch, b)
    d_v = torch.empty((1, r, r, n), dtype=torch.int64, device="cuda")               # G1 = A B^T, read as r vectors of width r
    d_g = torch.empty((1, r * (r + 1) // 2, n), dtype=torch.int64, device="cuda")   # G2 = the symmetric Gram matrix of G1's rows
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ctx.ring_gram_device(d_v.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), 1, r, r, width, s1.cuda_stream)
    ctx.ring_gram_device(d_g.data_ptr(), d_v.data_ptr(), 0, 1, r, r, r, s2.cuda_stream)
    s2.synchronize()
    s1.synchronize()
    v = _dot_route(ctx, a, b).reshape(1, r, r, n)
    assert np.array_equal(_host(d_v), v)
    assert np.array_equal(_host(d_g), _dot_route(ctx, v, None))
    ctx.close()


def test_graph_capture_after_eager_warm_up(pkg):
    """The Gram call needs the context's workspace at every n, so n = 64 reaches the path."""
    import torch
    q, n, batch, ra, rb, width = Q_NORTH, 64, 2, 2, 3, 2
    rng = np.random.default_rng(73)
    ctx = pkg.NttContext(q, n, device=0)
    d_a = torch.zeros((batch, ra, width, n), dtype=torch.int64, device="cuda")
    d_b = torch.zeros((batch, rb, width, n), dtype=torch.int64, device="cuda")
    d_g = torch.empty((batch, ra, rb, n), dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):      # eager warm-up: allocates the workspace
        ctx.ring_gram_device(d_g.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), batch, ra, rb, width, side.cuda_stream)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ctx.ring_gram_device(d_g.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), batch, ra, rb, width, torch.cuda.current_stream().cuda_stream)
    for _ in range(2):                 # two replays, each on fresh inputs
        a, b = _rand(rng, q, (batch, ra, width, n)), _rand(rng, q, (batch, rb, width, n))
        d_a.copy_(_dev(torch, a))
        d_b.copy_(_dev(torch, b))
        graph.replay()
        torch.cuda.synchronize()
        assert _host(d_g).tolist() == schoolbook_gram(a, b, q, -1)
    ctx.close()


def test_first_call_under_capture_is_refused(pkg):
    import torch
    q, n, batch, r, width = Q_NORTH, 64, 2, 2, 2
    rng = np.random.default_rng(74)
    ctx = pkg.NttContext(q, n, device=0)
    a = _rand(rng, q, (batch, r, width, n))
    d_a = _dev(torch, a)
    d_g = torch.zeros((batch, r * (r + 1) // 2, n), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    rc = None
    with torch.cuda.graph(graph, stream=side):
        d_g.add_(0)                    # (keeps the captured graph non-empty)
        rc = ctx._lib.lsr_ntt_ring_gram_batch_device(ctx.handle, d_g.data_ptr(), d_a.data_ptr(), None, batch, r, r, width,
                                                     torch.cuda.current_stream().cuda_stream)
    assert rc == -1
    assert "eager" in pkg._abi.last_error()
    graph.replay()                     # the capture stayed usable
    torch.cuda.synchronize()
    assert not bool(d_g.any())         # and holds no launch of the refused call
    ctx.ring_gram_device(d_g.data_ptr(), d_a.data_ptr(), None, batch, r, r, width, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert _host(d_g).tolist() == schoolbook_gram(a, None, q, -1)      # the context still works
    ctx.close()


# ---- 8. the empty batch ----------------------------------------------------------------------------------------------------------------
def test_empty_batch_writes_nothing(pkg):
    import torch
    n = 256
    ctx = pkg.NttContext(Q_NORTH, n, device=0)
    d = torch.full((3, n), SENTINEL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.current_stream().cuda_stream
    ctx.ring_gram_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 0, 2, 3, 2, s)
    ctx.ring_gram_device(d[0].data_ptr(), d[1].data_ptr(), None, 0, 2, 2, 2, s)
    torch.cuda.synchronize()
    assert bool((d == SENTINEL).all())
    empty = np.zeros((0, 2, 3, n), dtype=np.uint64)
    assert ctx.ring_gram(empty, empty).shape == (0, 2, 2, n)
    assert ctx.ring_gram(empty).shape == (0, 3, n)
    ctx.close()
