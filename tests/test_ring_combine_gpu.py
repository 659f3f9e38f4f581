"""GPU suite: the ring-element linear combination of commitment rows (lsr_lwe_ring_combine_rows_device,
lsr_lwe_ring_combine_batch_flat) against the model of tests/ring_combine_model.py word for word, against the scalar combine for constant
polynomials, through decode and verify, across the re-centring period, at the budget boundary, on malformed terms, on refused
arguments and under stream ordering."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ring_combine_model as model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIGMA = 3.19
KEY = 77
BASE_ROWS = 18                      # committed rows per context: (outputs - 1) * (terms + 1) + terms for outputs = 3, terms = 5

_CONTEXTS = {}
_BASE = {}


def _ctx(pkg, kind, n, k):
    key = (kind, n, k)
    if key not in _CONTEXTS:
        if kind == "rns":
            _CONTEXTS[key] = pkg.LweContext.create_rns(pkg.Params(n=n, k=k, sigma=SIGMA), key_seed=KEY)
        elif kind == "wide":
            _CONTEXTS[key] = pkg.LweContext(pkg.Params(q=pkg.wide_modulus(n), n=n, k=k, sigma=SIGMA), key_seed=KEY)
        else:
            _CONTEXTS[key] = pkg.LweContext(pkg.Params(n=n, k=k, sigma=SIGMA), key_seed=KEY)
    return _CONTEXTS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for ctx in _CONTEXTS.values():
        ctx.close()
    _CONTEXTS.clear()
    _BASE.clear()


def _moduli(ctx):
    return tuple(ctx.rns_moduli() or (ctx.commit_modulus,))


def _base(pkg, kind, n, k, rows=BASE_ROWS):
    """committed rows of the context (Commitment.batch_words) and their messages over all n slots, once per module"""
    key = (kind, n, k)
    if key not in _BASE:
        ctx = _ctx(pkg, kind, n, k)
        rng = np.random.default_rng(n + 7 * k)
        msgs = rng.integers(0, ctx.plain_modulus, size=(rows, n), dtype=np.uint64)
        seeds = rng.integers(1, 2**63, size=rows, dtype=np.uint64)
        _BASE[key] = (np.ascontiguousarray(pkg.Commitment.batch_words(ctx, msgs, seeds), dtype=np.uint64), msgs)
    return _BASE[key]


def _to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _buffers(ctx, polys):
    """(polynomials, output rows, status) on the device, filled on the current stream"""
    import torch
    polys = np.ascontiguousarray(polys, dtype=np.uint64)
    return (_to_device(polys), torch.full((polys.shape[0], ctx.commitment_words), -1, dtype=torch.int64, device="cuda"),
            torch.full((polys.shape[0],), 77, dtype=torch.int32, device="cuda"))


def _launch(ctx, d_rows, buffers, terms, term_stride, stream):
    d_polys, d_out, d_status = buffers
    ctx.ring_combine_rows_device(d_rows.data_ptr(), terms, d_polys.data_ptr(), d_out.shape[0], d_out.data_ptr(), d_status.data_ptr(), term_stride=term_stride,
                                 stream=stream)


def _device(ctx, d_rows, polys, term_stride):
    """d_rows: device tensor of rows; polys uint64 [outputs][terms][n] -> (out rows, status)"""
    import torch
    buffers = _buffers(ctx, polys)
    _launch(ctx, d_rows, buffers, polys.shape[1], term_stride, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return buffers[1].cpu().numpy().view(np.uint64), buffers[2].cpu().numpy()


def _both(ctx, rows, polys, term_stride):
    """the device entry point and the host one on the same rows, asserted equal where the status is 1 -> (out rows, status)"""
    outputs, terms = polys.shape[:2]
    used = np.ascontiguousarray(rows[:(outputs - 1) * term_stride + terms])
    dev = _device(ctx, _to_device(used), polys, term_stride)
    flat = ctx.ring_combine_rows(used, polys, term_stride=term_stride)
    assert np.array_equal(flat[1], dev[1])
    good = dev[1] == 1
    assert np.array_equal(flat[0][good], dev[0][good])
    return dev


def _sparse(rng, ctx, outputs, terms, n, every_word=True):
    """4 - 8 taps per polynomial out of the words 0, 1, t - 1, (t - 1)/2, (t + 1)/2, t + 5 and 2^64 - 1.  A tap of (t - 1)/2 alone
    weighs about 2^19, which the budget of a 44-bit default context (a weight of a few hundred) refuses by the contract's own rule, so
    there the taps of magnitude ~ t/2 are confined to polynomial (0, 0) (every_word; that output then has status 0 and its neighbours
    are checked to be unaffected) and every other polynomial draws from the words of small magnitude."""
    t = ctx.plain_modulus
    special = [0, 1, t - 1, (t - 1) // 2, (t + 1) // 2, t + 5, 2**64 - 1]
    roomy = terms * 8 * (t // 2) <= ctx.combine_max_weight
    pool = np.array(special if roomy else [c for c in special + [2, t - 2, 3 * t + 1] if abs(model.combine_model.centred(c, t)) <= 5], dtype=np.uint64)
    polys = np.zeros((outputs, terms, n), dtype=np.uint64)
    for j in range(outputs):
        for i in range(terms):
            taps = rng.choice(n, size=int(rng.integers(4, 9)), replace=False)
            polys[j, i, taps] = rng.choice(pool, size=taps.size)
    if every_word:
        polys[0, 0, :] = 0
        polys[0, 0, [0, 1, n // 2, n - 1, 5, 6, 7]] = np.array(special, dtype=np.uint64)   # every word, at the ends of the polynomial too
    return polys


def _verdicts(ctx, polys):
    """the status the budget rule gives each output: 1 when its exact weight is within combine_max_weight"""
    return [1 if model.weight(p, ctx.plain_modulus) <= ctx.combine_max_weight else 0 for p in polys]


# (1024, 2): 3 outputs x 3 components = 9 polynomials at 4 per tile, so the last tile is ragged and shares its only polynomial's
# output with the tile before it; (rns, 8192, 1): the large-magnitude words through the composed form
CONTEXTS = [("default", 4096, 2), ("rns", 4096, 1), ("default", 1024, 3), ("rns", 1024, 3), ("default", 8192, 2), ("wide", 4096, 2),
            ("default", 1024, 2), ("rns", 1024, 2), ("rns", 8192, 1)]


@pytest.mark.parametrize("kind,n,k", CONTEXTS)
def test_words_against_the_model(pkg, kind, n, k):
    ctx = _ctx(pkg, kind, n, k)
    base, _ = _base(pkg, kind, n, k)
    t, moduli = ctx.plain_modulus, _moduli(ctx)
    rng = np.random.default_rng(3 * n + k)
    outputs = 3
    for terms in (1, 2, 5):
        polys = _sparse(rng, ctx, outputs, terms, n)
        verdicts = _verdicts(ctx, polys)
        assert verdicts == ([0, 1, 1] if kind == "default" else [1, 1, 1])
        good = np.array(verdicts) == 1
        for stride in (0, terms, terms + 1):
            got, status = _both(ctx, base, polys, stride)
            assert status.tolist() == verdicts, (terms, stride)
            want = model.combine_rows(base, polys, stride, t, n, k, moduli)
            assert np.array_equal(got[good], want[good]), (terms, stride)


def test_words_against_the_model_at_two_pass_degree_65536(pkg):
    kind, n, k = "default", 65536, 1
    ctx = _ctx(pkg, kind, n, k)
    base, _ = _base(pkg, kind, n, k, rows=2)
    t = ctx.plain_modulus
    polys = _sparse(np.random.default_rng(9), ctx, 1, 2, n, every_word=False)
    got, status = _both(ctx, base, polys, 0)
    assert status.tolist() == [1]
    assert np.array_equal(got, model.combine_rows(base, polys, 0, t, n, k, _moduli(ctx)))


@pytest.mark.parametrize("kind,n,k", [("default", 4096, 2), ("rns", 1024, 3)])
def test_constant_polynomials_equal_the_scalar_combine(pkg, kind, n, k):
    import torch
    ctx = _ctx(pkg, kind, n, k)
    base, _ = _base(pkg, kind, n, k)
    t = ctx.plain_modulus
    outputs, terms = 3, 5
    W = ctx.combine_max_weight
    top = 2**64 - 1 if kind == "rns" else 3 * t + 1          # any 64-bit word; on the default context one of small magnitude mod t
    coeffs = np.array([[0, 1, t - 1, t + 2, top], [3, t - 2, 0, 2 * t, 1], [min(W, t // 2) + 1 if kind == "default" else 1, t // 2, 1, 1, 1]], dtype=np.uint64)
    polys = np.zeros((outputs, terms, n), dtype=np.uint64)
    polys[:, :, 0] = coeffs
    polys[1, 2, 17] = t                                      # 0 mod t: still a constant
    for stride in (0, terms):
        used = base[:(outputs - 1) * stride + terms]
        d_rows, d_coeffs = _to_device(used), _to_device(coeffs)
        d_out = torch.full((outputs, ctx.commitment_words), -1, dtype=torch.int64, device="cuda")
        d_status = torch.full((outputs,), 77, dtype=torch.int32, device="cuda")
        ctx.combine_rows_device(d_rows.data_ptr(), terms, d_coeffs.data_ptr(), outputs, d_out.data_ptr(), d_status.data_ptr(), term_stride=stride,
                                stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        want, want_status = d_out.cpu().numpy().view(np.uint64), d_status.cpu().numpy()
        got, status = _device(ctx, d_rows, polys, stride)
        assert np.array_equal(status, want_status), stride
        assert want_status.tolist() == ([1, 1, 0] if kind == "default" else [1, 1, 1])
        good = want_status == 1
        assert np.array_equal(got[good], want[good]), stride


@pytest.mark.parametrize("kind,n,k", [("default", 4096, 2), ("rns", 1024, 3), ("default", 8192, 2)])
def test_outputs_open_to_the_ring_combination_of_the_messages(pkg, kind, n, k):
    import torch
    ctx = _ctx(pkg, kind, n, k)
    base, msgs = _base(pkg, kind, n, k)
    t = ctx.plain_modulus
    rng = np.random.default_rng(5 * n + k)
    outputs, terms, stride = 3, 2, 2
    polys = _sparse(rng, ctx, outputs, terms, n, every_word=kind == "rns")
    got, status = _device(ctx, _to_device(base[:(outputs - 1) * stride + terms]), polys, stride)
    assert status.tolist() == [1] * outputs
    want = np.array([model.message(msgs[j * stride:j * stride + terms], polys[j], t) for j in range(outputs)], dtype=np.uint64)
    decoded, decode_status, bits = ctx.decode_rows(got, noise=True)
    print("noise bits", bits.tolist(), "capacity", ctx.noise_capacity_bits)
    assert decode_status.tolist() == [1] * outputs
    assert np.array_equal(decoded, want)
    assert all(int(b) < ctx.noise_capacity_bits for b in bits)
    wrong = want.copy()
    wrong[1, n // 3] = (int(wrong[1, n // 3]) + 1) % t
    d_rows, d_res = _to_device(got), torch.zeros(outputs, dtype=torch.int32, device="cuda")
    for claimed, verdict in ((want, [1, 1, 1]), (wrong, [1, 0, 1])):
        d_msgs = _to_device(claimed)
        ctx.verify_rows_device(d_rows.data_ptr(), d_msgs.data_ptr(), n, outputs, d_res.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert d_res.cpu().tolist() == verdict


def test_dense_polynomials_across_the_recentring_period(pkg, oracle):
    """identical term rows, every coefficient (t - 1)/2, on, just over and twice over the re-centring period of the accumulator"""
    kind, n, k = "rns", 1024, 3
    ctx = _ctx(pkg, kind, n, k)
    base, _ = _base(pkg, kind, n, k)
    t, moduli = ctx.plain_modulus, _moduli(ctx)
    for terms in (32, 33, 65):
        rows = np.repeat(base[:1], terms, axis=0)
        polys = np.full((1, terms, n), (t - 1) // 2, dtype=np.uint64)
        assert model.weight(polys, t) < ctx.combine_max_weight
        got, status = _both(ctx, rows, polys, 0)
        assert status.tolist() == [1], terms
        assert np.array_equal(got[0], model.combine_row(rows, polys[0], t, n, k, moduli, oracle=oracle)), terms


def test_budget_boundary(pkg):
    import torch
    kind, n, k = "default", 4096, 2
    ctx = _ctx(pkg, kind, n, k)
    base, _ = _base(pkg, kind, n, k)
    t, moduli = ctx.plain_modulus, _moduli(ctx)
    W = ctx.combine_max_weight
    assert 2 < W < n and W < t // 2
    polys = np.zeros((4, 1, n), dtype=np.uint64)
    polys[0, 0, :W] = 1                                       # weight W
    polys[1, 0, :W + 1] = 1                                   # weight W + 1
    polys[2, 0, n - W:] = t - 1                               # weight W, negative representatives
    polys[3, 0, [1, n - 1]] = [2, t - 3]                      # a neighbour of the refused output
    got, status = _both(ctx, base, polys, 1)
    assert status.tolist() == [1, 0, 1, 1]
    for j in (0, 2, 3):
        assert np.array_equal(got[j], model.combine_row(base[j:j + 1], polys[j], t, n, k, moduli)), j
    # the same W + 1 polynomial is far inside the budget of the RNS context
    rns = _ctx(pkg, "rns", 4096, 1)
    rns_base, _ = _base(pkg, "rns", 4096, 1)
    assert rns.combine_max_weight > 2**40
    got, status = _both(rns, rns_base, polys[1:2], 0)
    assert status.tolist() == [1]
    assert np.array_equal(got[0], model.combine_row(rns_base[:1], polys[1], t, 4096, 1, _moduli(rns)))
    # W itself against the scalar combine
    d_rows, d_coeffs = _to_device(base[:1]), _to_device(np.array([[W], [W + 1]], dtype=np.uint64))
    d_out = torch.zeros((2, ctx.commitment_words), dtype=torch.int64, device="cuda")
    d_status = torch.full((2,), 77, dtype=torch.int32, device="cuda")
    ctx.combine_rows_device(d_rows.data_ptr(), 1, d_coeffs.data_ptr(), 2, d_out.data_ptr(), d_status.data_ptr(), term_stride=0,
                            stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert d_status.cpu().tolist() == [1, 0]


@pytest.mark.parametrize("kind,n,k", [("default", 4096, 2), ("rns", 1024, 3), ("default", 1024, 3), ("default", 8192, 2)])
def test_malformed_term_rows(pkg, kind, n, k):
    """one bad term of output 1 in a call of three disjoint groups: status [1, -1, 1], the good rows as in the clean run"""
    ctx = _ctx(pkg, kind, n, k)
    other_kind = "default" if kind == "rns" else "rns"
    base, _ = _base(pkg, kind, n, k)
    t, moduli = ctx.plain_modulus, _moduli(ctx)
    head, blocks = model.layout(n, k, moduli)
    rng = np.random.default_rng(n + 11 * k)
    outputs, terms = 3, 2
    polys = _sparse(rng, ctx, outputs, terms, n, every_word=kind == "rns")
    clean_rows = base[:outputs * terms].copy()
    clean, clean_status = _both(ctx, clean_rows, polys, terms)
    assert clean_status.tolist() == [1] * outputs
    victim = terms + 1
    foreign = np.zeros(ctx.commitment_words, dtype=np.uint64)
    row = _base(pkg, other_kind, n, k)[0][0]
    width = min(foreign.size, row.size)
    foreign[:width] = row[:width]                 # a row of the other kind of context, truncated or zero-padded to this row length
    last_first, last_words, last_q = blocks[-1]
    edits = [("magic", lambda r: r.__setitem__(1, int(r[1]) ^ 1)), ("body word == q", lambda r: r.__setitem__(last_first + last_words // 2 + 3, last_q)),
             ("foreign row", lambda r: r.__setitem__(slice(None), foreign))]
    for name, edit in edits:
        rows = clean_rows.copy()
        edit(rows[victim])
        got, status = _both(ctx, rows, polys, terms)
        assert status.tolist() == [1, -1, 1], name
        assert np.array_equal(got[[0, 2]], clean[[0, 2]]), name


def test_refusals_leave_the_context_usable(pkg, lib):
    import torch
    kind, n, k = "default", 1024, 3
    ctx = _ctx(pkg, kind, n, k)
    base, msgs = _base(pkg, kind, n, k)
    W = ctx.commitment_words
    d_rows = _to_device(base[:4])
    d_polys = torch.zeros((2, 2, n), dtype=torch.int64, device="cuda")
    d_out = torch.full((2, W), -1, dtype=torch.int64, device="cuda")
    d_status = torch.full((2,), 77, dtype=torch.int32, device="cuda")
    h, s = ctx.handle, torch.cuda.current_stream().cuda_stream
    r, p, o, st = d_rows.data_ptr(), d_polys.data_ptr(), d_out.data_ptr(), d_status.data_ptr()
    dev = lib.lsr_lwe_ring_combine_rows_device
    refused = [lambda: dev(h, r, 0, 2, p, 2, o, st, s), lambda: dev(h, r, pkg._abi.RING_COMBINE_MAX_TERMS + 1, 0, p, 2, o, st, s),
               lambda: dev(h, r, 2, 2, p, 2, r, st, s), lambda: dev(h, r, 2, 2, p, 2, p, st, s), lambda: dev(h, r, 2, 2, p, 2**31, o, st, s),
               lambda: dev(h, r, 2, 2**62, p, 3, o, st, s), lambda: dev(h, None, 2, 2, p, 2, o, st, s)]
    for call in refused:
        assert not lib.lsr_lwe_context_create_rns(None, 3, -1) and b"NULL params" in lib.lsr_last_error()      # another text in between
        assert call() == -1
        assert b"lsr_lwe_ring_combine_rows_device" in lib.lsr_last_error(), lib.lsr_last_error()
    host = np.ascontiguousarray(base[:4])
    status = np.full(2, 77, dtype=np.int32)
    for terms in (0, pkg._abi.RING_COMBINE_MAX_TERMS + 1):
        assert lib.lsr_lwe_ring_combine_batch_flat(h, host.ctypes.data, terms, 0, host.ctypes.data, 2, host.ctypes.data + 8, status.ctypes.data) == -1
        assert b"lsr_lwe_ring_combine_batch_flat" in lib.lsr_last_error()
    assert dev(h, r, 2, 2, p, 0, o, st, s) == 0
    torch.cuda.synchronize()
    assert d_status.cpu().tolist() == [77, 77] and bool((d_out == -1).all().item())                           # nothing was written
    # the context commits and opens afterwards
    rows = np.ascontiguousarray(pkg.Commitment.batch_words(ctx, msgs[:2], np.array([5, 6], dtype=np.uint64)), dtype=np.uint64)
    decoded, decode_status = ctx.decode_rows(rows)
    assert decode_status.tolist() == [1, 1] and np.array_equal(decoded, msgs[:2])


def test_calls_on_two_streams_are_ordered(pkg):
    """two calls on two streams of one context, then a decode of the second call's output on the first stream, with no synchronisation by
    the caller: the results of sequential calls"""
    import torch
    kind, n, k = "default", 4096, 2
    ctx = _ctx(pkg, kind, n, k)
    base, msgs = _base(pkg, kind, n, k)
    t = ctx.plain_modulus
    rng = np.random.default_rng(13)
    batch, terms = 8, 2
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    d_rows = _to_device(base[:batch + 1])
    for it in range(5):
        polys_a, polys_b = _sparse(rng, ctx, batch, terms, n, every_word=False), _sparse(rng, ctx, batch, terms, n, every_word=False)
        want_a, status_a = _device(ctx, d_rows, polys_a, 1)
        want_b, status_b = _device(ctx, d_rows, polys_b, 1)
        assert status_a.tolist() == [1] * batch and status_b.tolist() == [1] * batch
        want_msgs, _ = ctx.decode_rows(want_b)
        d_msgs = torch.zeros((batch, n), dtype=torch.int64, device="cuda")
        d_dstatus = torch.zeros(batch, dtype=torch.int32, device="cuda")
        buffers_a, buffers_b = _buffers(ctx, polys_a), _buffers(ctx, polys_b)
        (_, out_a, st_a), (_, out_b, st_b) = buffers_a, buffers_b
        torch.cuda.synchronize()                 # every fill above is complete before the side streams start
        _launch(ctx, d_rows, buffers_a, terms, 1, streams[0].cuda_stream)
        _launch(ctx, d_rows, buffers_b, terms, 1, streams[1].cuda_stream)
        ctx.decode_rows_device(out_b.data_ptr(), batch, n, d_msgs.data_ptr(), d_dstatus.data_ptr(), None, streams[0].cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(out_a.cpu().numpy().view(np.uint64), want_a), it
        assert np.array_equal(out_b.cpu().numpy().view(np.uint64), want_b), it
        assert st_a.cpu().tolist() == [1] * batch and st_b.cpu().tolist() == [1] * batch
        assert d_dstatus.cpu().tolist() == [1] * batch and np.array_equal(d_msgs.cpu().numpy().view(np.uint64), want_msgs), it


_CHUNKED = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as entry
pkg = entry.load_package()
data = np.load(sys.argv[2] + "/in.npz")
results = {}
for name in str(data["names"]).split(","):
    kind, n, k, stride = name.split("_")[0], int(data[name + "_n"]), int(data[name + "_k"]), int(data[name + "_stride"])
    params = pkg.Params(n=n, k=k, sigma=float(data["sigma"]))
    ctx = pkg.LweContext.create_rns(params, key_seed=int(data["key"])) if kind == "rns" else pkg.LweContext(params, key_seed=int(data["key"]))
    polys = data[name + "_polys"]
    outputs, terms = polys.shape[:2]
    d_rows = torch.from_numpy(data[name + "_rows"].view(np.int64)).cuda()
    d_polys = torch.from_numpy(polys.view(np.int64)).cuda()
    d_out = torch.full((outputs, ctx.commitment_words), -1, dtype=torch.int64, device="cuda")
    d_status = torch.full((outputs,), 77, dtype=torch.int32, device="cuda")
    ctx.ring_combine_rows_device(d_rows.data_ptr(), terms, d_polys.data_ptr(), outputs, d_out.data_ptr(), d_status.data_ptr(), term_stride=stride,
                                 stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    results[name + "_out"] = d_out.cpu().numpy().view(np.uint64)
    results[name + "_status"] = d_status.cpu().numpy()
    ctx.close()
np.savez(sys.argv[2] + "/out.npz", **results)
"""


def _few_taps(rng, t, outputs, terms, n):
    """2 - 3 taps of +-1 per polynomial (as 1, t - 1, t + 1): 200 terms stay inside the budget of a 44-bit context"""
    polys = np.zeros((outputs, terms, n), dtype=np.uint64)
    for j in range(outputs):
        for i in range(terms):
            taps = rng.choice(n, size=int(rng.integers(2, 4)), replace=False)
            polys[j, i, taps] = rng.choice(np.array([1, t - 1, t + 1], dtype=np.uint64), size=taps.size)
    return polys


def test_groups_of_terms_and_chunks_of_outputs_under_a_small_workspace(pkg, tmp_path):
    """LAMBDA_SNARK_NTT_CHUNK_MIB=1 (read once per process: a fresh child) shrinks the workspace to 32 polynomials at n = 4096, 64 per
    prime on the RNS context at n = 1024 and 4 terms at (8192, 2).  Words against the model for
      default (4096, 2): 2 outputs of 70 terms = groups of 32 + 32 + 6 with the raw accumulator waiting in the output row, one output
                         per pass; 8 outputs of 5 terms = chunks of 6 + 2 outputs;
      rns (1024, 3):     2 outputs of 130 terms = groups of 64 + 64 + 2; 15 outputs of 5 terms = chunks of 12 + 3;
      default (8192, 2): 2 outputs of 9 terms = groups of 4 + 4 + 1, the partial results added."""
    cases = [("default_a", 4096, 2, 2, 70, 1), ("default_b", 4096, 2, 8, 5, 1), ("rns_a", 1024, 3, 2, 130, 0), ("rns_b", 1024, 3, 15, 5, 1),
             ("default_c", 8192, 2, 2, 9, 2)]
    rng = np.random.default_rng(71)
    blob, want = {"names": ",".join(c[0] for c in cases), "sigma": SIGMA, "key": KEY}, {}
    for name, n, k, outputs, terms, stride in cases:
        kind = name.split("_")[0]
        ctx = _ctx(pkg, kind, n, k)
        base, _ = _base(pkg, kind, n, k)
        t = ctx.plain_modulus
        rows = base[np.arange((outputs - 1) * stride + terms) % BASE_ROWS]
        polys = _sparse(rng, ctx, outputs, terms, n, every_word=False) if kind == "rns" else _few_taps(rng, t, outputs, terms, n)
        assert _verdicts(ctx, polys) == [1] * outputs
        blob.update({name + "_n": n, name + "_k": k, name + "_stride": stride, name + "_rows": rows, name + "_polys": polys})
        want[name] = model.combine_rows(rows, polys, stride, t, n, k, _moduli(ctx))
    np.savez(str(tmp_path / "in.npz"), **blob)
    script = tmp_path / "chunked.py"
    script.write_text(_CHUNKED)
    subprocess.run([sys.executable, str(script), ROOT, str(tmp_path)], check=True, env=dict(os.environ, LAMBDA_SNARK_NTT_CHUNK_MIB="1"), timeout=300)
    out = np.load(str(tmp_path / "out.npz"))
    for name, _, _, outputs, _, _ in cases:
        assert out[name + "_status"].tolist() == [1] * outputs, name
        assert np.array_equal(out[name + "_out"], want[name]), name
