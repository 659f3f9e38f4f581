"""GPU suite: the ring quadratic forms out[j] = sum_i g_ii c_i^2 + offdiag sum_{i<l} g_il c_i c_l (lsr_ntt_ring_quadform_batch / _device)
and the symmetrised packed Gram matrix h_il = <a_i, b_l> + <a_l, b_i> (lsr_ntt_ring_gram_sym2_batch / _device), DESIGN.md §5m.
Pinned against the schoolbook definitions, word for word against the composed routes (ring product per pair, scaling, ring inner
product; ring inner products per pair added mod q) in every arithmetic flavour, at the accumulators' worst case and on either side
of the FP64 re-centring period, in where the outputs land, under a shrunken workspace (groups of pairs, family chunks, column
groups), in the refusals that read the context, in the device form across streams and under graph capture, and in the verifier's
two closing identities of a folded witness.
The sweep against models that share nothing with the library, in every flavour, lives in tests/test_ring_gram_sweep_gpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from ring_gram_model import packed_index
from ring_quadform_model import composed_quadform, composed_sym2, schoolbook_quadform_parts, schoolbook_sym2
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


def _from_parts(parts, q, offdiag):
    diag, off = parts
    return [[(d + offdiag * o) % q for d, o in zip(dj, oj)] for dj, oj in zip(diag, off)]


# ---- 1. schoolbook ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [12289, Q_NORTH])
@pytest.mark.parametrize("n", [2, 16, 256])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("r", [1, 2, 5])
def test_quadform_matches_schoolbook(pkg, q, n, batch, r):
    rng = np.random.default_rng(n + 10 * r + 100 * batch + q % 1000)
    ctx = pkg.NttContext(q, n, device=0)
    g = _rand(rng, q, (batch, r * (r + 1) // 2, n))
    for c in (_rand(rng, q, (r, n)), _rand(rng, q, (batch, r, n))):            # c_rows == 1 (the 2-d form) and c_rows == batch
        parts = schoolbook_quadform_parts(g, c, q, -1)
        for offdiag in (1, 2, (q + 1) // 2):
            assert ctx.ring_quadform(g, c, offdiag).tolist() == _from_parts(parts, q, offdiag), (q, n, batch, r, c.ndim, offdiag)
    assert ctx.ring_quadform(g[0], c[0], 2).tolist() == _from_parts(parts, q, 2)[0]     # a 2-d g: a batch of one
    ctx.close()


@pytest.mark.parametrize("q", [12289, Q_NORTH])
@pytest.mark.parametrize("n", [2, 16, 256])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("shape", [(1, 1), (2, 5), (3, 2)])
def test_sym2_matches_schoolbook(pkg, q, n, batch, shape):
    r, width = shape
    rng = np.random.default_rng(n + 10 * r + 100 * batch + q % 1000 + 1)
    ctx = pkg.NttContext(q, n, device=0)
    a, b = _rand(rng, q, (batch, r, width, n)), _rand(rng, q, (batch, r, width, n))
    assert ctx.ring_gram_sym2(a, b).tolist() == schoolbook_sym2(a, b, q, -1), (q, n, batch, shape)
    assert ctx.ring_gram_sym2(a, a).tolist() == schoolbook_sym2(a, a, q, -1), (q, n, batch, shape, "b is a")
    assert ctx.ring_gram_sym2(a[0], b[0]).tolist() == schoolbook_sym2(a[:1], b[:1], q, -1)[0]      # 3-d operands: a batch of one
    ctx.close()


def test_cyclic_goldilocks_matches_plain_convolution(pkg):
    n = 16
    rng = np.random.default_rng(16)
    ntt = pkg.CyclicNtt(n)
    for batch in (1, 3):
        for r in (1, 2, 5):
            g = _rand(rng, GOLD, (batch, r * (r + 1) // 2, n))
            for c in (_rand(rng, GOLD, (r, n)), _rand(rng, GOLD, (batch, r, n))):
                parts = schoolbook_quadform_parts(g, c, GOLD, 1)
                for offdiag in (1, 2, (GOLD + 1) // 2):
                    assert ntt.ring_quadform(g, c, offdiag).tolist() == _from_parts(parts, GOLD, offdiag), (batch, r, c.ndim, offdiag)
        for r, width in [(1, 1), (2, 5), (3, 2)]:
            a, b = _rand(rng, GOLD, (batch, r, width, n)), _rand(rng, GOLD, (batch, r, width, n))
            assert ntt.ring_gram_sym2(a, b).tolist() == schoolbook_sym2(a, b, GOLD, 1), (batch, r, width)
            assert ntt.ring_gram_sym2(a, a).tolist() == schoolbook_sym2(a, a, GOLD, 1), (batch, r, width)
    ntt.close()


# ---- 2. word for word against the composed routes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", ["f64", "u64_q60", "u64_q44"])
@pytest.mark.parametrize("n", [256, 4096, 8192, 65536])
@pytest.mark.parametrize("call", ["quadform", "sym2"])
def test_equals_the_composed_route(pkg, lib, flavour, n, call):
    """r = 1, E, E + 1, 2 E + 1 with E = ring_gram_block (sym2: below one block, one diagonal block, a diagonal and an off-diagonal
    block with partial blocks of each kind; the quadratic form: one row, and triangles that the slices cut inside rows)."""
    batch = 2 if n < 65536 else 1
    q, ctx = _flavour_context(pkg, lib, flavour, n)
    e = ctx.ring_gram_block
    assert e >= 2
    rng = np.random.default_rng(n + len(flavour) + len(call))
    big = n < 8192 or flavour == "f64"                         # 2 E + 1 at n >= 8192: one flavour
    for r in [1, e, e + 1] + ([2 * e + 1] if big else []):
        if call == "quadform":
            g = _rand(rng, q, (batch, r * (r + 1) // 2, n))
            for c, offdiag in [(_rand(rng, q, (batch, r, n)), 2), (_rand(rng, q, (1, r, n)), 1)]:
                assert np.array_equal(ctx.ring_quadform(g, c, offdiag), composed_quadform(ctx, q, g, c, offdiag)), (flavour, n, r, offdiag)
        else:
            a, b = _rand(rng, q, (batch, r, 2, n)), _rand(rng, q, (batch, r, 2, n))
            assert np.array_equal(ctx.ring_gram_sym2(a, b), composed_sym2(ctx, q, a, b)), (flavour, n, r)
    ctx.close()


def test_largest_two_pass_degree(pkg):
    n, q, r = 1 << 17, Q44, 2
    rng = np.random.default_rng(17)
    ctx = pkg.NttContext(q, n, device=0)
    g, c = _rand(rng, q, (1, 3, n)), _rand(rng, q, (1, r, n))
    assert np.array_equal(ctx.ring_quadform(g, c, 2), composed_quadform(ctx, q, g, c, 2))
    a, b = _rand(rng, q, (1, r, 1, n)), _rand(rng, q, (1, r, 1, n))
    assert np.array_equal(ctx.ring_gram_sym2(a, b), composed_sym2(ctx, q, a, b))
    ctx.close()


# ---- 3. the accumulators ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [31, 32, 33, 64])
def test_quadform_f64_rows_on_both_sides_of_the_recentring_period(pkg, r):
    """A row of the triangle has up to r - 1 off-diagonal products and a slice up to r rows: 31, 32, 33 sit on either side of the
    period of the inner and of the outer sum, 64 is the most vectors (2080 pairs a position: the slicing engages).  Random operands
    and all-(q - 1) operands, whose every product and sum is as large as it can be."""
    assert pkg.RING_DOT_F64_RECENTRE_PERIOD == 32
    n, q = 256, Q_NORTH
    rng = np.random.default_rng(r)
    ctx = pkg.NttContext(q, n, device=0)
    assert ctx.uses_f64
    npairs = r * (r + 1) // 2
    for g, c in [(_rand(rng, q, (2, npairs, n)), _rand(rng, q, (2, r, n))),
                 (np.full((1, npairs, n), q - 1, dtype=np.uint64), np.full((1, r, n), q - 1, dtype=np.uint64))]:
        for offdiag in (2, q - 1):
            assert np.array_equal(ctx.ring_quadform(g, c, offdiag), composed_quadform(ctx, q, g, c, offdiag)), (r, offdiag)
    ctx.close()


@pytest.mark.parametrize("flavour", ["f64", "u64_q60"])
def test_quadform_many_slices_of_one_workgroup_of_positions(pkg, lib, flavour):
    n, r = 16, 64
    q, ctx = _flavour_context(pkg, lib, flavour, n)
    rng = np.random.default_rng(64)
    npairs = r * (r + 1) // 2
    for g, c in [(_rand(rng, q, (1, npairs, n)), _rand(rng, q, (1, r, n))),
                 (np.full((1, npairs, n), q - 1, dtype=np.uint64), np.full((1, r, n), q - 1, dtype=np.uint64))]:
        assert np.array_equal(ctx.ring_quadform(g, c, 2), composed_quadform(ctx, q, g, c, 2)), flavour
    ctx.close()


def test_quadform_goldilocks_sums_are_reduced(pkg):
    n, r = 256, 33
    ntt = pkg.CyclicNtt(n)
    npairs = r * (r + 1) // 2
    g, c = np.full((1, npairs, n), GOLD - 1, dtype=np.uint64), np.full((1, r, n), GOLD - 1, dtype=np.uint64)
    assert np.array_equal(ntt.ring_quadform(g, c, GOLD - 1), composed_quadform(ntt, GOLD, g, c, GOLD - 1))
    ntt.close()


@pytest.mark.parametrize("width", [15, 16, 17, 33])
def test_sym2_f64_recentring_period_on_both_sides(pkg, width):
    """Two products a column: the running sums are re-centred every 16 columns."""
    n, q = 256, Q_NORTH
    rng = np.random.default_rng(width)
    ctx = pkg.NttContext(q, n, device=0)
    assert ctx.uses_f64
    r = ctx.ring_gram_block + 1                      # a diagonal block, an off-diagonal block, partial blocks
    for a, b in [(_rand(rng, q, (2, r, width, n)), _rand(rng, q, (2, r, width, n))),
                 (np.full((1, r, width, n), q - 1, dtype=np.uint64), np.full((1, r, width, n), q - 1, dtype=np.uint64))]:
        assert np.array_equal(ctx.ring_gram_sym2(a, b), composed_sym2(ctx, q, a, b)), width
    ctx.close()


# ---- 4. where the outputs land ---------------------------------------------------------------------------------------------------------
def test_outputs_land_in_their_buffers_and_operands_are_unchanged(pkg):
    import torch
    n, q, batch, width = 256, Q_NORTH, 2, 2
    ctx = pkg.NttContext(q, n, device=0)
    r = ctx.ring_gram_block + 1
    outs = r * (r + 1) // 2
    rng = np.random.default_rng(41)
    a, b, c = _rand(rng, q, (batch, r, width, n)), _rand(rng, q, (batch, r, width, n)), _rand(rng, q, (batch, r, n))
    d_a, d_b, d_c = _dev(torch, a), _dev(torch, b), _dev(torch, c)
    d_h = torch.full((batch * outs + 1, n), SENTINEL, dtype=torch.int64, device="cuda")          # one polynomial more than the call owns
    d_out = torch.full((batch + 1, n), SENTINEL, dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    ctx.ring_gram_sym2_device(d_h.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), batch, r, width, s)
    torch.cuda.synchronize()
    h = _host(d_h)
    d_g = _dev(torch, h[:-1])
    ctx.ring_quadform_device(d_out.data_ptr(), d_g.data_ptr(), d_c.data_ptr(), batch, r, batch, 1, s)
    torch.cuda.synchronize()
    out, sentinel = _host(d_out), np.uint64(SENTINEL)
    assert (h[-1] == sentinel).all() and (out[-1] == sentinel).all()
    assert (h[:-1] < q).all() and (out[:-1] < q).all()                   # every owned word was written (the sentinel is above q)
    assert np.array_equal(_host(d_a), a) and np.array_equal(_host(d_b), b) and np.array_equal(_host(d_c), c)
    assert np.array_equal(_host(d_g), h[:-1])
    want_h = composed_sym2(ctx, q, a, b)
    assert np.array_equal(h[:-1].reshape(batch, outs, n), want_h)
    assert np.array_equal(out[:-1], composed_quadform(ctx, q, want_h, c, 1))
    assert np.array_equal(ctx.ring_quadform(want_h, c, 1), out[:-1])      # the host form
    ctx.close()


# ---- 5. groups of pairs, family chunks and column groups under a shrunken workspace ------------------------------------------------------
_CHUNKED = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as entry
import ring_quadform_model as t
pkg = entry.load_package()
data = np.load(sys.argv[2] + "/in.npz")
q = int(data["q"])
out = {}
for name, n, kind in [tuple(c) for c in data["cases"].tolist()]:
    ctx = pkg.NttContext(q, int(n), device=0)
    x, y = data[name + "_x"], data[name + "_y"]
    if kind == "quadform":
        out[name + "_got"] = ctx.ring_quadform(x, y, 2)
        out[name + "_composed"] = t.composed_quadform(ctx, q, x, y, 2)
    else:
        out[name + "_got"] = ctx.ring_gram_sym2(x, y)
        out[name + "_composed"] = t.composed_sym2(ctx, q, x, y)
    ctx.close()
# r + 2 = 9 polynomials against the 8 of the workspace at n = 65536: refused, and nothing is written
n = 65536
ctx = pkg.NttContext(q, n, device=0)
g, c = np.zeros((1, 28, n), dtype=np.uint64), np.zeros((1, 7, n), dtype=np.uint64)
res = np.full((1, n), 7, dtype=np.uint64)
rc = ctx._lib.lsr_ntt_ring_quadform_batch(ctx.handle, res.ctypes.data, g.ctypes.data, c.ctypes.data, 1, 7, 1, 2)
out["refused_rc"] = np.int64(rc)
out["refused_message"] = np.array(pkg._abi.last_error())
out["refused_untouched"] = np.bool_((res == 7).all())
out["allowed_rc"] = np.int64(ctx._lib.lsr_ntt_ring_quadform_batch(ctx.handle, res.ctypes.data, g.ctypes.data, c.ctypes.data, 1, 6, 1, 2))
ctx.close()
np.savez(sys.argv[2] + "/out.npz", **out)
"""

# (name, n, kind, batch, r, c_rows or width): under LAMBDA_SNARK_NTT_CHUNK_MIB=6 the workspace holds 64 polynomials at n = 4096 and 8 at 2^16
_CHUNK_SHAPES = [
    ("pair_groups", 4096, "quadform", 2, 12, 2),       # 12 + 78 > 64: c-hat resident, g in groups of pairs that end inside rows
    ("family_chunks", 4096, "quadform", 9, 3, 1),      # a shared c, 6 pairs + 2 partials a family against 61: chunks of 7 + 2 families
    ("pair_groups_65536", 65536, "quadform", 2, 3, 2),   # 3 + 6 > 8: groups of 4 + 2 pairs
    ("family_chunks_65536", 65536, "quadform", 3, 2, 1),   # a shared c, 3 pairs a family against 6: chunks of 2 + 1 families
    ("sym2_column_groups", 4096, "sym2", 2, 3, 14),    # (3 + 3) * 14 = 84 > 64: groups of 10 + 4 columns
]


def test_groups_and_chunks_equal_the_unchunked_result(pkg, tmp_path):
    """LAMBDA_SNARK_NTT_CHUNK_MIB is read once per process: a fresh child.  The child's results are compared with its own composed
    routes and with this process's results under the full workspace."""
    q = Q44
    rng = np.random.default_rng(56)
    arrays, cases, want = {}, [], {}
    for name, n, kind, batch, r, last in _CHUNK_SHAPES:
        ctx = pkg.NttContext(q, n, device=0)
        if kind == "quadform":
            x, y = _rand(rng, q, (batch, r * (r + 1) // 2, n)), _rand(rng, q, (last, r, n))
            want[name] = ctx.ring_quadform(x, y, 2)
        else:
            x, y = _rand(rng, q, (batch, r, last, n)), _rand(rng, q, (batch, r, last, n))
            want[name] = ctx.ring_gram_sym2(x, y)
        arrays[name + "_x"], arrays[name + "_y"] = x, y
        cases.append((name, str(n), kind))
        ctx.close()
    np.savez(str(tmp_path / "in.npz"), q=np.uint64(q), cases=np.array(cases), **arrays)
    script = tmp_path / "chunked.py"
    script.write_text(_CHUNKED)
    subprocess.run([sys.executable, str(script), ROOT, str(tmp_path)], check=True, env=dict(os.environ, LAMBDA_SNARK_NTT_CHUNK_MIB="6"), timeout=300)
    out = np.load(str(tmp_path / "out.npz"))
    for name, _, _ in cases:
        assert np.array_equal(out[name + "_got"], out[name + "_composed"]), name
        assert np.array_equal(out[name + "_got"], want[name]), name
    assert int(out["refused_rc"]) == -1
    assert "LAMBDA_SNARK_NTT_CHUNK_MIB" in str(out["refused_message"]) and "lsr_ntt_ring_quadform_batch:" in str(out["refused_message"])
    assert bool(out["refused_untouched"])
    assert int(out["allowed_rc"]) == 0                  # r + 2 = 8 polynomials: the workspace is just enough


# ---- 6. the refusals that read the context ---------------------------------------------------------------------------------------------
def test_offdiag_must_be_canonical(pkg):
    n, q = 64, Q_NORTH
    ctx = pkg.NttContext(q, n, device=0)
    g, c = np.zeros((1, 3, n), dtype=np.uint64), np.zeros((1, 2, n), dtype=np.uint64)
    for offdiag in (q, q + 1, (1 << 64) - 1):
        with pytest.raises(pkg.CoreError):
            ctx.ring_quadform(g, c, offdiag)
        msg = pkg._abi.last_error()
        assert "offdiag" in msg and "lsr_ntt_ring_quadform_batch:" in msg
    assert ctx.ring_quadform(g, c, q - 1).shape == (1, n)
    ctx.close()


def test_output_overlapping_an_operand_is_refused(pkg):
    import torch
    n, batch, r, width = 256, 2, 3, 2
    ctx = pkg.NttContext(Q_NORTH, n, device=0)
    g_polys, c_polys, a_polys = batch * r * (r + 1) // 2, batch * r, batch * r * width
    buf = torch.zeros((a_polys + g_polys, n), dtype=torch.int64, device="cuda")
    other = torch.zeros((a_polys, n), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.current_stream().cuda_stream
    fn = ctx._lib.lsr_ntt_ring_quadform_batch_device
    # out straddling the operand's end / out on the operand's first rows / out right behind the operand (allowed)
    for row, rc_want in [(g_polys - 1, -1), (0, -1), (g_polys, 0)]:
        assert fn(ctx.handle, buf[row].data_ptr(), buf.data_ptr(), other.data_ptr(), batch, r, batch, 2, s) == rc_want, ("g", row)
        msg = pkg._abi.last_error()
        assert rc_want == 0 or ("overlaps g" in msg and "lsr_ntt_ring_quadform_batch_device" in msg)
    for row, rc_want in [(c_polys - 1, -1), (0, -1), (c_polys, 0)]:
        assert fn(ctx.handle, buf[row].data_ptr(), other.data_ptr(), buf.data_ptr(), batch, r, batch, 2, s) == rc_want, ("c", row)
        msg = pkg._abi.last_error()
        assert rc_want == 0 or ("overlaps c" in msg and "lsr_ntt_ring_quadform_batch_device" in msg)
    # a shared c owns r polynomials
    assert fn(ctx.handle, buf[r - 1].data_ptr(), other.data_ptr(), buf.data_ptr(), batch, r, 1, 2, s) == -1
    assert fn(ctx.handle, buf[r].data_ptr(), other.data_ptr(), buf.data_ptr(), batch, r, 1, 2, s) == 0
    fn2 = ctx._lib.lsr_ntt_ring_gram_sym2_batch_device
    for row, rc_want in [(a_polys - 1, -1), (0, -1), (a_polys, 0)]:
        assert fn2(ctx.handle, buf[row].data_ptr(), buf.data_ptr(), other.data_ptr(), batch, r, width, s) == rc_want, ("a", row)
        msg = pkg._abi.last_error()
        assert rc_want == 0 or ("overlaps a" in msg and "lsr_ntt_ring_gram_sym2_batch_device" in msg)
        assert fn2(ctx.handle, buf[row].data_ptr(), other.data_ptr(), buf.data_ptr(), batch, r, width, s) == rc_want, ("b", row)
        msg = pkg._abi.last_error()
        assert rc_want == 0 or ("overlaps b" in msg and "lsr_ntt_ring_gram_sym2_batch_device" in msg)
    torch.cuda.synchronize()
    host = np.zeros((g_polys + batch, n), dtype=np.uint64)
    assert ctx._lib.lsr_ntt_ring_quadform_batch(ctx.handle, host[1].ctypes.data, host.ctypes.data, host.ctypes.data, batch, r, batch, 2) == -1
    assert "lsr_ntt_ring_quadform_batch:" in pkg._abi.last_error()
    ctx.close()


def test_context_above_two_pass_sizes_is_refused(pkg):
    ntt = pkg.CyclicNtt(1 << 18)
    x = np.zeros((1, 1, 1 << 18), dtype=np.uint64)
    with pytest.raises(pkg.CoreError):
        ntt.ring_quadform(x, x, 2)
    assert "131072" in pkg._abi.last_error()
    with pytest.raises(pkg.CoreError):
        ntt.ring_gram_sym2(x[None], x[None])
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
    out, g, c = (small[k].data_ptr() for k in range(3))
    assert 64 * 65 // 2 * n * 8 > MAX_FAMILY_BYTES and (64 + 64) * 32 * n * 8 > MAX_FAMILY_BYTES
    assert ctx._lib.lsr_ntt_ring_quadform_batch_device(ctx.handle, out, g, c, 1, 64, 1, 2, s) == -1
    msg = pkg._abi.last_error()
    assert "LSR_RING_GRAM_MAX_FAMILY_BYTES" in msg and "lsr_ntt_ring_quadform_batch_device" in msg
    for width in (32, 1):              # the operands of a family; its packed outputs
        assert ctx._lib.lsr_ntt_ring_gram_sym2_batch_device(ctx.handle, out, g, c, 1, 64, width, s) == -1
        msg = pkg._abi.last_error()
        assert "LSR_RING_GRAM_MAX_FAMILY_BYTES" in msg and "lsr_ntt_ring_gram_sym2_batch_device" in msg
    torch.cuda.synchronize()
    assert bool((small == SENTINEL).all())
    ctx.close()


# ---- 7. the device form ------------------------------------------------------------------------------------------------------------
def test_device_form_is_ordered_across_streams(pkg):
    """sym2 on one stream writes the h that the quadratic form on another stream reads, with no synchronisation between them, and
    both transform their operands into the one workspace of the context.  The context's ring event orders the two."""
    import torch
    q, n, r, width = Q44, 65536, 3, 2
    rng = np.random.default_rng(n + 9)
    ctx = pkg.NttContext(q, n, device=0)
    a, b, c = _rand(rng, q, (1, r, width, n)), _rand(rng, q, (1, r, width, n)), _rand(rng, q, (1, r, n))
    d_a, d_b, d_c = _dev(torch, a), _dev(torch, b), _dev(torch, c)
    d_h = torch.empty((1, r * (r + 1) // 2, n), dtype=torch.int64, device="cuda")
    d_out = torch.empty((1, n), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ctx.ring_gram_sym2_device(d_h.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), 1, r, width, s1.cuda_stream)
    ctx.ring_quadform_device(d_out.data_ptr(), d_h.data_ptr(), d_c.data_ptr(), 1, r, 1, 1, s2.cuda_stream)
    s2.synchronize()
    s1.synchronize()
    h = composed_sym2(ctx, q, a, b)
    assert np.array_equal(_host(d_h), h)
    assert np.array_equal(_host(d_out), composed_quadform(ctx, q, h, c, 1))
    ctx.close()


def test_graph_capture_after_eager_warm_up(pkg):
    """Both calls need the context's workspace at every n, so n = 64 reaches the path; r = 8 at batch 2 runs several slices."""
    import torch
    q, n, batch, r, width = Q_NORTH, 64, 2, 8, 2
    npairs = r * (r + 1) // 2
    rng = np.random.default_rng(75)
    ctx = pkg.NttContext(q, n, device=0)
    d_a = torch.zeros((batch, r, width, n), dtype=torch.int64, device="cuda")
    d_b = torch.zeros((batch, r, width, n), dtype=torch.int64, device="cuda")
    d_c = torch.zeros((1, r, n), dtype=torch.int64, device="cuda")
    d_h = torch.empty((batch, npairs, n), dtype=torch.int64, device="cuda")
    d_out = torch.empty((batch, n), dtype=torch.int64, device="cuda")

    def enqueue(stream):
        ctx.ring_gram_sym2_device(d_h.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), batch, r, width, stream)
        ctx.ring_quadform_device(d_out.data_ptr(), d_h.data_ptr(), d_c.data_ptr(), batch, r, 1, 1, stream)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):      # eager warm-up: allocates the workspace
        enqueue(side.cuda_stream)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        enqueue(torch.cuda.current_stream().cuda_stream)
    for _ in range(2):                 # two replays, each on fresh inputs
        a, b, c = _rand(rng, q, (batch, r, width, n)), _rand(rng, q, (batch, r, width, n)), _rand(rng, q, (1, r, n))
        d_a.copy_(_dev(torch, a))
        d_b.copy_(_dev(torch, b))
        d_c.copy_(_dev(torch, c))
        graph.replay()
        torch.cuda.synchronize()
        h = composed_sym2(ctx, q, a, b)
        assert np.array_equal(_host(d_h), h)
        assert np.array_equal(_host(d_out), composed_quadform(ctx, q, h, c, 1))
    ctx.close()


@pytest.mark.parametrize("call", ["quadform", "sym2"])
def test_first_call_under_capture_is_refused(pkg, call):
    import torch
    q, n, batch, r, width = Q_NORTH, 64, 2, 2, 2
    rng = np.random.default_rng(76)
    ctx = pkg.NttContext(q, n, device=0)
    x = _rand(rng, q, (batch, 3, n)) if call == "quadform" else _rand(rng, q, (batch, r, width, n))
    c = _rand(rng, q, (batch, r, n))
    d_x, d_c = _dev(torch, x), _dev(torch, c)
    d_res = torch.zeros((batch, 1 if call == "quadform" else 3, n), dtype=torch.int64, device="cuda")

    def enqueue(stream):
        if call == "quadform":
            return ctx._lib.lsr_ntt_ring_quadform_batch_device(ctx.handle, d_res.data_ptr(), d_x.data_ptr(), d_c.data_ptr(), batch, r, batch, 2, stream)
        return ctx._lib.lsr_ntt_ring_gram_sym2_batch_device(ctx.handle, d_res.data_ptr(), d_x.data_ptr(), d_x.data_ptr(), batch, r, width, stream)

    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    rc = None
    with torch.cuda.graph(graph, stream=side):
        d_res.add_(0)                  # (keeps the captured graph non-empty)
        rc = enqueue(torch.cuda.current_stream().cuda_stream)
    assert rc == -1
    assert "eager" in pkg._abi.last_error()
    graph.replay()                     # the capture stayed usable
    torch.cuda.synchronize()
    assert not bool(d_res.any())       # and holds no launch of the refused call
    assert enqueue(torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    want = composed_quadform(ctx, q, x, c, 2)[:, None] if call == "quadform" else composed_sym2(ctx, q, x, x)
    assert np.array_equal(_host(d_res), want)      # the context still works
    ctx.close()


def test_empty_batch_writes_nothing(pkg):
    import torch
    n = 256
    ctx = pkg.NttContext(Q_NORTH, n, device=0)
    d = torch.full((3, n), SENTINEL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.current_stream().cuda_stream
    ctx.ring_quadform_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 0, 2, 1, 2, s)
    ctx.ring_gram_sym2_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 0, 2, 2, s)
    torch.cuda.synchronize()
    assert bool((d == SENTINEL).all())
    assert ctx.ring_quadform(np.zeros((0, 3, n), dtype=np.uint64), np.zeros((2, n), dtype=np.uint64)).shape == (0, n)
    assert ctx.ring_gram_sym2(np.zeros((0, 2, 3, n), dtype=np.uint64), np.zeros((0, 2, 3, n), dtype=np.uint64)).shape == (0, 3, n)
    ctx.close()


# ---- 8. the verifier's closing identities, exact --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 4096])
def test_verifier_identities_of_a_folded_witness(pkg, n):
    """z = sum_i c_i s_i with c from the BALL sampler:  <z, z> = sum g_il c_i c_l over the packed g = ring_gram(s) with offdiag = 2, and
    sum_i <phi_i, z> c_i = <sum_i c_i phi_i, z> = sum h_il c_i c_l over h = ring_gram_sym2(phi, s) with offdiag = 1."""
    q, r, width, kappa = Q_NORTH, 5, 3, 16
    rng = np.random.default_rng(n + 5)
    ctx = pkg.NttContext(q, n, device=0)
    s, phi = _rand(rng, q, (r, width, n)), _rand(rng, q, (r, width, n))
    c = ctx.ring_sample(r, pkg.RING_SAMPLE_BALL, kappa, pkg.ring_sample_key(0xC0FFEE + n))
    assert [int(np.count_nonzero(p)) for p in c] == [kappa] * r
    z = ctx.ring_fold(s, c)
    assert z.shape == (width, n)
    assert np.array_equal(ctx.ring_quadform(ctx.ring_gram(s), c, 2), ctx.ring_dot(z, z))
    assert np.array_equal(ctx.ring_quadform(ctx.ring_gram_sym2(phi, s), c, 1), ctx.ring_dot(ctx.ring_fold(phi, c), z))
    assert pkg.ring_gram_index(r, 1, 3) == packed_index(r, 1, 3)
    ctx.close()
