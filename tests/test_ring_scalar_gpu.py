"""GPU suite: the scalar-weighted aggregation of ring vectors with an addend (lsr_ntt_ring_scalar_combine_batch and its _device form,
DESIGN.md §5l) word for word against the Python-integer model of tests/ring_scalar_model.py, in the host and the device form, with no
addend, a separate one and the in-place one, on every kind of context; at the term counts where the kernel re-centres, restages and
carries; with planted weights (all q - 1, a word = q, 2^64 - 1, 2^52 + 1); against the library's own fold, projection, back-projection
and inner products; with buffers off 16-byte alignment (one position per lane instead of two); in the refusals that read the context;
and under graph capture with no warm-up call.

Nothing here feeds a non-canonical word of v or addend to the device: the rule about them (an unspecified result, never a fault) is
covered by reading the kernel, which only does arithmetic on the words it loads."""
import os
import re

import numpy as np
import pytest

import ring_scalar_model as model
from ring_norm_model import ROWS, key_from_seed
from test_ring_matvec_gpu import _flavour_context

pytestmark = pytest.mark.gpu

Q14 = 12289
GOLD = 18446744069414584321
CONTEXTS = ["q14", "f64", "u64_q44", "u64_q60", "gold"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HEADER = open(os.path.join(ROOT, "include", "lambda_snark", "batch.h")).read()
TILE = int(re.search(r"#define\s+LSR_RING_SCALAR_COMBINE_TILE\s+(\d+)", _HEADER).group(1))       # positions per workgroup, two per lane
STAGE = int(re.search(r"#define\s+LSR_RING_SCALAR_COMBINE_STAGE\s+(\d+)", _HEADER).group(1))     # weights staged at a time
# (n, width).  A length is width n with n >= 2, so it is even: TILE - 2 and TILE + 2 are the lengths next to the tile, TILE is the tile.
EDGES = [(2, TILE // 2 - 1), (2, TILE // 2), (2, TILE // 2 + 1)]
# buffers off 16-byte alignment take one position per lane and half the tile
EDGES_OFF = [(2, TILE // 4 - 1), (2, TILE // 4), (2, TILE // 4 + 1)]
SHAPES = [(2, 1), (8, 5), (64, 5), (256, 3), (4096, 2)] + EDGES
SETS = [1, 3, 5, 16]           # one; the protocol's three; five; the most (each runs the kernel's instantiation for exactly its sets)
PATTERN = 0x5A5A5A5A5A5A5A5A   # the device outputs before the call: an unwritten word shows


def _context(pkg, lib, kind, n):
    if kind == "q14":
        return Q14, pkg.NttContext(Q14, n, device=0)
    if kind == "gold":
        return GOLD, pkg.CyclicNtt(n)
    return _flavour_context(pkg, lib, kind, n)


def _rand(rng, q, shape):
    return rng.integers(0, q, size=shape, dtype=np.uint64)


def _dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()


def _dev_off(torch, x, words):
    """x on the device, `words` 8-byte words behind a 16-byte boundary."""
    flat = torch.empty(x.size + 2, dtype=torch.int64, device="cuda")
    view = flat[words:words + x.size].view(x.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(x).view(np.int64)))
    assert view.data_ptr() % 16 == 8 * words
    return view


def _plus(want, addend, q):
    """(want + addend) mod q in Python integers."""
    total = (np.array(want.tolist(), dtype=object) + np.array(addend.tolist(), dtype=object)) % q
    return np.array(total.tolist(), dtype=np.uint64).reshape(want.shape)


def _device_call(ctx, v, weights, addend, count, ts, components, in_place):
    """The device form on outputs pre-filled with PATTERN (in place: with the addend; status: 7) -> (out, status list)."""
    import torch
    sets, terms, width = weights.shape[1], weights.shape[2], v.shape[1]
    d_v, d_w = _dev(torch, v), _dev(torch, weights)
    d_status = torch.full((count,), 7, dtype=torch.int32, device="cuda")
    if in_place:
        d_out = _dev(torch, addend)
        d_add = d_out
    else:
        d_out = torch.full((count, sets, width, ctx.n), PATTERN, dtype=torch.int64, device="cuda")
        d_add = None if addend is None else _dev(torch, addend)
    torch.cuda.synchronize()
    ctx.ring_scalar_combine_device(d_out.data_ptr(), d_status.data_ptr(), d_v.data_ptr(), d_w.data_ptr(), 0 if d_add is None else d_add.data_ptr(), count,
                                   sets, terms, ts, width, components, torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    if d_add is not None and not in_place:
        assert np.array_equal(d_add.cpu().numpy().view(np.uint64), addend)         # a separate addend is only read
    return d_out.cpu().numpy().view(np.uint64), d_status.cpu().tolist()


def _host_in_place(ctx, v, weights, addend, count, ts, components):
    out = np.ascontiguousarray(addend).copy()
    status = np.full(count, 7, dtype=np.int32)
    v3, w3 = np.ascontiguousarray(v), np.ascontiguousarray(weights)
    rc = ctx._lib.lsr_ntt_ring_scalar_combine_batch(ctx.handle, out.ctypes.data, status.ctypes.data, v3.ctypes.data, w3.ctypes.data, out.ctypes.data, count,
                                                    w3.shape[1], w3.shape[2], ts, v3.shape[1], components)
    assert rc == 0
    return out, status.tolist()


def _check_forms(ctx, v, weights, addend, count, ts, components, want, want_added, want_status, what):
    """Host and device form; no addend (`want`), and with `addend` separate and in place (`want_added`)."""
    got, status = ctx.ring_scalar_combine(v, weights, count, ts, components)
    assert got.dtype == np.uint64 and got.shape == want.shape and status.tolist() == want_status, what
    assert np.array_equal(got, want), ("host", what)
    got, status = _device_call(ctx, v, weights, None, count, ts, components, False)
    assert status == want_status and np.array_equal(got, want), ("device", what)
    if addend is None:
        return
    got, status = ctx.ring_scalar_combine(v, weights, count, ts, components, addend=addend)
    assert status.tolist() == want_status and np.array_equal(got, want_added), ("host, addend", what)
    got, status = _host_in_place(ctx, v, weights, addend, count, ts, components)
    assert status == want_status and np.array_equal(got, want_added), ("host, in place", what)
    for in_place in (False, True):
        got, status = _device_call(ctx, v, weights, addend, count, ts, components, in_place)
        assert status == want_status and np.array_equal(got, want_added), ("device, addend", in_place, what)


# ---- 1. shapes, word for word against the model -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", CONTEXTS)
@pytest.mark.parametrize("n,width", SHAPES)
def test_matches_the_model(pkg, lib, kind, n, width):
    """count 5 with components 2: a ragged last group, three weight groups; terms 3 with term_stride 0 (shared), 3 (disjoint), 5 (spaced)
    and 1 (overlapping); every sets of SETS; no addend, a separate one, the in-place one; the host and the device form.  The model
    runs once per term_stride, for 16 sets: fewer sets are its leading sets; the addend is added to its result in Python integers
    (held against the model's own addend at term_stride 0).  Q14 has no ring above n = 2048: there the longest shape keeps its length
    at n = 2048."""
    if kind == "q14" and n > 2048:
        n, width = 2048, n * width // 2048
    q, ctx = _context(pkg, lib, kind, n)
    count, components, terms = 5, 2, 3
    rng = np.random.default_rng(n + width)
    weights = _rand(rng, q, (3, 16, terms))
    addend = _rand(rng, q, (count, 16, width, n))
    for ts in (0, terms, terms + 2, 1):
        v = _rand(rng, q, ((count - 1) * ts + terms, width, n))
        want, want_status = model.scalar_combine(q, n, width, v, weights, None, count, ts, components)
        assert want_status.tolist() == [1] * count and want.any()
        added = _plus(want, addend, q)
        if ts == 0:
            assert np.array_equal(added, model.scalar_combine(q, n, width, v, weights, addend, count, ts, components)[0])
        for sets in SETS:
            w = np.ascontiguousarray(weights[:, :sets])
            _check_forms(ctx, v, w, np.ascontiguousarray(addend[:, :sets]), count, ts, components, want[:, :sets], added[:, :sets], [1] * count,
                         (kind, n, width, ts, sets))
    ctx.close()


@pytest.mark.parametrize("kind", CONTEXTS)
@pytest.mark.parametrize("n,width", [(64, 5)] + EDGES_OFF + EDGES)
def test_buffers_off_sixteen_bytes(pkg, lib, kind, n, width):
    """The device form with v, out, the addend — one of them, or all — one word behind a 16-byte boundary: one position per lane, 8-byte
    accesses, half the tile.  sets 3 and 16, a separate addend and the in-place one (which moves with out)."""
    import torch
    q, ctx = _context(pkg, lib, kind, n)
    count, components, terms = 3, 2, 3
    rng = np.random.default_rng(n * width)
    v, weights, addend = _rand(rng, q, (count * terms, width, n)), _rand(rng, q, (2, 16, terms)), _rand(rng, q, (count, 16, width, n))
    want, _ = model.scalar_combine(q, n, width, v, weights, addend, count, terms, components)
    stream = torch.cuda.current_stream().cuda_stream
    for sets in (3, 16):
        w, a = np.ascontiguousarray(weights[:, :sets]), np.ascontiguousarray(addend[:, :sets])
        d_w = _dev(torch, w)
        for off_v, off_out, off_add in [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (0, 1, None), (1, 0, None)]:      # None: in place
            d_v = _dev_off(torch, v, off_v)
            d_out = _dev_off(torch, a if off_add is None else np.full_like(a, PATTERN), off_out)
            d_add = d_out if off_add is None else _dev_off(torch, a, off_add)
            d_status = torch.full((count,), 7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            ctx.ring_scalar_combine_device(d_out.data_ptr(), d_status.data_ptr(), d_v.data_ptr(), d_w.data_ptr(), d_add.data_ptr(), count, sets, terms, terms,
                                           width, components, stream)
            torch.cuda.current_stream().synchronize()
            assert d_status.cpu().tolist() == [1] * count
            assert np.array_equal(d_out.cpu().numpy().view(np.uint64), want[:, :sets]), (kind, n, width, sets, off_v, off_out, off_add)
    ctx.close()


# ---- 2. term counts at the reduction boundaries -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", CONTEXTS)
@pytest.mark.parametrize("terms", [1, 31, 32, 33, 64, 65, STAGE + 1, 2 * STAGE + 33])
def test_term_counts_at_the_reduction_boundaries(pkg, lib, kind, terms):
    """len 40, sets 5, two outputs over overlapping terms (term_stride 1).  Random words; and ALL of v, weights and addend q - 1 —
    the largest products and sums there are: (q - 1)^2 = 1, so every word is terms mod q, or terms - 1 with the addend."""
    n, width, sets, count = 8, 5, 5, 2
    q, ctx = _context(pkg, lib, kind, n)
    rng = np.random.default_rng(terms)
    v, weights, addend = _rand(rng, q, (terms + 1, width, n)), _rand(rng, q, (1, sets, terms)), _rand(rng, q, (count, sets, width, n))
    want, _ = model.scalar_combine(q, n, width, v, weights, None, count, 1, 2)
    added, _ = model.scalar_combine(q, n, width, v, weights, addend, count, 1, 2)
    _check_forms(ctx, v, weights, addend, count, 1, 2, want, added, [1, 1], (kind, terms, "random"))
    v, weights, addend = np.full_like(v, q - 1), np.full_like(weights, q - 1), np.full_like(addend, q - 1)
    want, _ = model.scalar_combine(q, n, width, v, weights, None, count, 1, 2)
    added, _ = model.scalar_combine(q, n, width, v, weights, addend, count, 1, 2)
    assert set(want.reshape(-1).tolist()) == {terms % q} and set(added.reshape(-1).tolist()) == {(terms - 1) % q}
    _check_forms(ctx, v, weights, addend, count, 1, 2, want, added, [1, 1], (kind, terms, "q - 1"))
    ctx.close()


# ---- 3. status --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,bad", [(kind, bad) for kind in CONTEXTS for bad in ("q", 2**64 - 1)] + [("f64", 2**52 + 1)])
def test_a_weight_not_below_q_refuses_its_group_only(pkg, lib, kind, bad):
    """A weight = q, 2^64 - 1 or (FP64 flavour) 2^52 + 1, whose low 52 bits are canonical, in the last set of the middle group: status
    -1 and zeros for exactly that group's vectors, in place included; the others as without it."""
    n, width, count, sets, terms = 64, 5, 5, 3, 4
    q, ctx = _context(pkg, lib, kind, n)
    rng = np.random.default_rng(5)
    v, weights, addend = _rand(rng, q, (count * terms, width, n)), _rand(rng, q, (3, sets, terms)), _rand(rng, q, (count, sets, width, n))
    weights[1, sets - 1, 2] = q if bad == "q" else bad
    want, want_status = model.scalar_combine(q, n, width, v, weights, None, count, terms, 2)
    added, _ = model.scalar_combine(q, n, width, v, weights, addend, count, terms, 2)
    assert want_status.tolist() == [1, 1, -1, -1, 1] and not want[2:4].any() and not added[2:4].any() and want[0].any() and want[4].any()
    _check_forms(ctx, v, weights, addend, count, terms, 2, want, added, want_status.tolist(), (kind, bad))
    ctx.close()


# ---- 4. long and large ------------------------------------------------------------------------------------------------------------------
def test_one_long_vector(pkg, lib):
    n = 1 << 16                                                   # 256 tiles of one element
    q, ctx = _flavour_context(pkg, lib, "f64", n)
    rng = np.random.default_rng(16)
    v, weights, addend = _rand(rng, q, (2, 1, n)), _rand(rng, q, (1, 3, 2)), _rand(rng, q, (1, 3, 1, n))
    want, _ = model.scalar_combine(q, n, 1, v, weights, None, 1, 0, 1)
    _check_forms(ctx, v, weights, addend, 1, 0, 1, want, _plus(want, addend, q), [1], "n = 2^16")
    ctx.close()


def test_large_cyclic_context_matches_the_model(pkg):
    n = 1 << 18                                                   # the smallest n above 2^17
    ctx = pkg.CyclicNtt(n)
    rng = np.random.default_rng(18)
    v, weights, addend = _rand(rng, GOLD, (2, 1, n)), _rand(rng, GOLD, (1, 1, 2)), _rand(rng, GOLD, (1, 1, 1, n))
    want, _ = model.scalar_combine(GOLD, n, 1, v, weights, None, 1, 0, 1)
    _check_forms(ctx, v, weights, addend, 1, 0, 1, want, _plus(want, addend, GOLD), [1], "n = 2^18")
    ctx.close()


# ---- 5. against the library's own calls -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f64", "gold"])
def test_equals_the_fold_by_constant_polynomials(pkg, lib, kind):
    """One ring_fold_device per set with every scalar dressed up as a constant polynomial, permuted on the host."""
    import torch
    n, width, count, sets, terms, components = 256, 3, 4, 3, 5, 2
    q, ctx = _context(pkg, lib, kind, n)
    rng = np.random.default_rng(256)
    v, weights = _rand(rng, q, (count * terms, width, n)), _rand(rng, q, (2, sets, terms))
    got, status = ctx.ring_scalar_combine(v, weights, count, terms, components)
    assert status.tolist() == [1] * count
    d_v = _dev(torch, v)
    stream = torch.cuda.current_stream().cuda_stream
    for k in range(sets):
        p = np.zeros((count, terms, n), dtype=np.uint64)
        p[:, :, 0] = weights[np.arange(count) // components, k]
        d_p = _dev(torch, p)
        d_out = torch.full((count, width, n), PATTERN, dtype=torch.int64, device="cuda")
        ctx.ring_fold_device(d_out.data_ptr(), d_v.data_ptr(), d_p.data_ptr(), count, terms, terms, width, stream)
        torch.cuda.current_stream().synchronize()
        assert np.array_equal(d_out.cpu().numpy().view(np.uint64), got[:, k]), k
    ctx.close()


@pytest.mark.parametrize("kind", ["f64", "gold"])
def test_the_aggregated_constraint_holds_end_to_end(pkg, lib, kind):
    """s sampled BOUNDED, p = Pi s, Pi^T w conjugated written by ring_project_adjoint_device, sum_l psi_l phi_l added in place by the
    new call on the same stream: the constant coefficient of <out_k, s> is sum_l psi^(k)_l ct<phi_l, s> + <w^(k), p> mod q."""
    import torch
    n, width, count, sets, terms, beta, index_base = 256, 3, 2, 3, 4, 1 << 10, 9
    q, ctx = _context(pkg, lib, kind, n)
    rng = np.random.default_rng(n + 5)
    key = np.array([key_from_seed(n + 44)], dtype=np.uint64)
    s = ctx.ring_sample(count * width, pkg.RING_SAMPLE_BOUNDED, beta, np.array([key_from_seed(7)], dtype=np.uint64)).reshape(count, width, n)
    p, p_status = ctx.ring_project(s, beta, key, components=count, index_base=index_base)
    assert p_status.tolist() == [1] * count and p.any()
    omega, psi, phi = _rand(rng, q, (1, sets, ROWS)), _rand(rng, q, (1, sets, terms)), _rand(rng, q, (count * terms, width, n))
    d_omega, d_psi, d_phi, d_key = _dev(torch, omega), _dev(torch, psi), _dev(torch, phi), _dev(torch, key)
    d_out = torch.full((count, sets, width, n), PATTERN, dtype=torch.int64, device="cuda")
    d_status = torch.full((2, count), 7, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ctx.ring_project_adjoint_device(d_out.data_ptr(), d_status[0].data_ptr(), d_omega.data_ptr(), count, sets, width, 1, d_key.data_ptr(), count, 17,
                                    index_base, stream)
    ctx.ring_scalar_combine_device(d_out.data_ptr(), d_status[1].data_ptr(), d_phi.data_ptr(), d_psi.data_ptr(), d_out.data_ptr(), count, sets, terms,
                                   terms, width, count, stream)
    torch.cuda.current_stream().synchronize()
    assert d_status.cpu().tolist() == [[1] * count] * 2
    out = d_out.cpu().numpy().view(np.uint64)
    for j in range(count):
        ct = [int(ctx.ring_dot(phi[j * terms + l], s[j])[0]) for l in range(terms)]
        for k in range(sets):
            want = (sum(int(psi[0, k, l]) * ct[l] for l in range(terms)) + sum(int(w) * int(x) for w, x in zip(omega[0, k].tolist(), p[j].tolist()))) % q
            assert int(ctx.ring_dot(out[j, k], s[j])[0]) == want, (j, k)
    ctx.close()


# ---- 6. the refusals that read the context ----------------------------------------------------------------------------------------------
def test_context_rules_are_refused(pkg, lib):
    n = 4096
    q, ctx = _flavour_context(pkg, lib, "f64", n)
    name = "lsr_ntt_ring_scalar_combine_batch"
    sets, terms = 2, 2
    weights = np.ones((1, sets, terms), dtype=np.uint64)
    v = np.ones((terms + 2, 1, n), dtype=np.uint64)
    out = np.zeros((2, sets, 1, n), dtype=np.uint64)               # room for an addend one word behind out[0]
    status = np.zeros(1, dtype=np.int32)

    def call(o, st, vv, w, addend, count=1, width=1):
        return ctx._lib.lsr_ntt_ring_scalar_combine_batch(ctx.handle, o, st, vv, w, addend, count, sets, terms, 0, width, 1)
    good = (out.ctypes.data, status.ctypes.data, v.ctypes.data, weights.ctypes.data)
    for count, width, needle in [(1, (1 << 20) + 1, "2^32"),       # width n above 2^32
                                 (1 << 48, 1, "overflow")]:         # count * sets * 16 fits, * n * 8 does not
        assert call(*good, None, count, width) == -1
        msg = pkg._abi.last_error()
        assert needle in msg and name + ":" in msg, msg
    # out may not share memory with v, weights, status — reported in that order — nor with an addend that is not out itself
    inside_v = v.ctypes.data + 8 * n
    assert call(inside_v, inside_v, v.ctypes.data, inside_v, inside_v + 8) == -1
    assert "out overlaps v" in pkg._abi.last_error() and name + ":" in pkg._abi.last_error()
    assert call(out.ctypes.data, out.ctypes.data, v.ctypes.data, out.ctypes.data + 64, out.ctypes.data + 8) == -1
    msg = pkg._abi.last_error()
    assert "out overlaps weights" in msg and "overlaps v" not in msg               # nothing left of the call before
    assert call(out.ctypes.data, out.ctypes.data + 64, v.ctypes.data, weights.ctypes.data, out.ctypes.data + 8) == -1
    msg = pkg._abi.last_error()
    assert "out overlaps status" in msg and "weights" not in msg
    out_bytes = 8 * sets * n
    for o, addend in [(out.ctypes.data, out.ctypes.data + 8), (out.ctypes.data, out.ctypes.data + out_bytes - 8),
                      (out[1].ctypes.data, out[1].ctypes.data - 8)]:        # an addend one word off out, on either side, or sharing one word
        assert call(o, *good[1:], addend) == -1
        msg = pkg._abi.last_error()
        assert "addend" in msg and "status" not in msg and name + ":" in msg
    # the same buffers apart and in place: served, 1 + 1 and then (1 + 1) + (1 + 1)
    assert call(*good, None) == 0 and status.tolist() == [1] and set(out[0].reshape(-1).tolist()) == {2}
    assert call(*good, out.ctypes.data) == 0 and status.tolist() == [1] and set(out[0].reshape(-1).tolist()) == {4}
    assert call(*good, out[1].ctypes.data) == 0 and set(out[0].reshape(-1).tolist()) == {2}      # out[1] is still 0
    # and the message of the next refusal is its own
    assert call(*good, None, 1, (1 << 20) + 1) == -1
    msg = pkg._abi.last_error()
    assert "2^32" in msg and "overlaps" not in msg
    ctx.close()


# ---- 7. graph capture with no warm-up call ----------------------------------------------------------------------------------------------
def test_graph_capture_from_the_first_call(pkg):
    """The first call this context ever sees is the captured one: one kernel on one stream; one replay equals the model."""
    import torch
    q, n, width, count, sets, terms = 17592180539393, 1024, 5, 3, 3, 4
    ctx = pkg.NttContext(q, n, device=0)
    rng = np.random.default_rng(1024)
    v, weights, addend = _rand(rng, q, (count + terms - 1, width, n)), _rand(rng, q, (2, sets, terms)), _rand(rng, q, (count, sets, width, n))
    d_v, d_w, d_add = _dev(torch, v), _dev(torch, weights), _dev(torch, addend)
    d_out = torch.full((count, sets, width, n), PATTERN, dtype=torch.int64, device="cuda")
    d_status = torch.full((count,), 7, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ctx.ring_scalar_combine_device(d_out.data_ptr(), d_status.data_ptr(), d_v.data_ptr(), d_w.data_ptr(), d_add.data_ptr(), count, sets, terms, 1,
                                       width, 2, torch.cuda.current_stream().cuda_stream)
    graph.replay()
    torch.cuda.synchronize()
    want, want_status = model.scalar_combine(q, n, width, v, weights, addend, count, 1, 2)
    assert d_status.cpu().tolist() == want_status.tolist() == [1, 1, 1]
    assert np.array_equal(d_out.cpu().numpy().view(np.uint64), want)
    ctx.close()
