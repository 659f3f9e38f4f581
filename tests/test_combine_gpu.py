"""GPU suite: the batched, device-resident linear combination of commitment rows (lsr_lwe_combine_rows_device,
lsr_lwe_combine_batch_flat) against lwe_linear_combine word for word, against the big-integer model of tests/combine_model.py at the
arithmetic extreme, at the budget boundary, through decode and verify, on malformed terms, and under stream ordering and graph capture."""
import ctypes

import numpy as np
import pytest

import combine_model

pytestmark = pytest.mark.gpu

SIGMA = 3.19
KEY = 77
MSG_LEN = 6
BASE_ROWS = 37                      # committed rows per context; longer term lists repeat them

_CONTEXTS = {}
_BASE = {}
_HOST = {}


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
    _HOST.clear()


def _layout(ctx):
    """(header words, [(first word, words, modulus)]) of a row of this context"""
    pair = ctx.rns_moduli()
    head, block = (6 if pair else 5), (ctx.module_rank + 1) * ctx.ring_degree
    return head, [(head + i * block, block, q) for i, q in enumerate(pair or (ctx.commit_modulus,))]


def _commit(ctx, msgs, seeds):
    msgs = np.ascontiguousarray(msgs, dtype=np.uint64)
    seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
    rows = np.zeros((seeds.size, ctx.commitment_words), dtype=np.uint64)
    assert ctx._lib.lsr_lwe_commit_batch_flat(ctx.handle, msgs.ctypes.data, msgs.shape[1], seeds.size, seeds.ctypes.data, rows.ctypes.data) == 0
    return rows


def _base(pkg, kind, n, k):
    """BASE_ROWS committed rows of the context and their messages, once per module"""
    key = (kind, n, k)
    if key not in _BASE:
        ctx = _ctx(pkg, kind, n, k)
        rng = np.random.default_rng(n + 7 * k)
        msgs = rng.integers(0, ctx.plain_modulus, size=(BASE_ROWS, MSG_LEN), dtype=np.uint64)
        _BASE[key] = (_commit(ctx, msgs, rng.integers(1, 2**63, size=BASE_ROWS, dtype=np.uint64)), msgs)
    return _BASE[key]


def _host_combine(pkg, ctx, rows, coeffs):
    """lwe_linear_combine on LweCommitment views of `rows` with the coefficient words as given -> data words, or None when refused"""
    rows = [np.ascontiguousarray(r) for r in rows]
    views = [pkg._abi.LweCommitment(r.ctypes.data_as(pkg._abi.u64p), r.size) for r in rows]
    arr = (ctypes.POINTER(pkg._abi.LweCommitment) * len(views))(*[ctypes.pointer(v) for v in views])
    cf = np.array([int(c) for c in coeffs], dtype=np.uint64)
    p = ctx._lib.lwe_linear_combine(ctx.handle, arr, cf.ctypes.data, len(views))
    if not p:
        return None
    out = np.ctypeslib.as_array(p.contents.data, shape=(p.contents.len,)).copy()
    ctx._lib.lwe_commitment_free(p)
    return out


def _host_reference(pkg, key, ctx, base, index, coeffs):
    """the same through a cache: (context, base row indices, coefficients) -> data words"""
    ident = (key, tuple(int(i) for i in index), tuple(int(c) for c in coeffs))
    if ident not in _HOST:
        _HOST[ident] = _host_combine(pkg, ctx, [base[i] for i in index], coeffs)
    return _HOST[ident]


def _combine_device(ctx, d_rows, coeffs, term_stride, stream=None):
    """d_rows: a device tensor of rows (int64 view); coeffs [outputs][terms] numpy -> (out rows, status)"""
    import torch
    coeffs = np.ascontiguousarray(coeffs, dtype=np.uint64)
    outputs, terms = coeffs.shape
    d_coeffs = torch.from_numpy(coeffs.view(np.int64)).cuda()
    d_out = torch.full((outputs, ctx.commitment_words), -1, dtype=torch.int64, device="cuda")
    d_status = torch.full((outputs,), 77, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    ctx.combine_rows_device(d_rows.data_ptr(), terms, d_coeffs.data_ptr(), outputs, d_out.data_ptr(), d_status.data_ptr(), term_stride=term_stride, stream=s)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(np.uint64), d_status.cpu().numpy()


def _to_device(rows):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rows).view(np.int64)).cuda()


def _both(ctx, rows, coeffs, term_stride):
    """the device entry point and the flat twin on the same rows, asserted equal where the status is 1 -> (out rows, status)"""
    coeffs = np.ascontiguousarray(coeffs, dtype=np.uint64)
    outputs, terms = coeffs.shape
    used = np.ascontiguousarray(rows[:(outputs - 1) * term_stride + terms])
    dev = _combine_device(ctx, _to_device(used), coeffs, term_stride)
    flat = ctx.combine_rows(used, coeffs, term_stride=term_stride)
    assert np.array_equal(flat[1], dev[1])
    good = dev[1] == 1
    assert np.array_equal(flat[0][good], dev[0][good])
    return dev


def _pool(ctx, kind):
    """coefficient words that stay inside the budget of every context when a few dozen of them are summed (|c'| <= 3), in every
    disguise: small positives, t - 1, t - 2, zero, and words >= t up to the top of the 64-bit range"""
    t = ctx.plain_modulus
    top = ((2**64 - 1) // t - 1) * t
    return [0, 1, 2, 3, t - 1, t - 2, t, t + 1, 3 * t + 2, 5 * t - 1, top + 1, top + t - 2]


def _draw(ctx, kind, rng, outputs, terms):
    t = ctx.plain_modulus
    if kind == "rns":               # the reference's range: any value below t (a few small and extreme ones mixed in)
        coeffs = rng.integers(0, t, size=(outputs, terms), dtype=np.uint64)
        special = np.array([0, 1, t - 1, t - 2, t // 2, t // 2 + 1], dtype=np.uint64)
        mask = rng.random((outputs, terms)) < 0.3
        coeffs[mask] = rng.choice(special, size=int(mask.sum()))
        return coeffs
    pool = np.array(_pool(ctx, kind), dtype=np.uint64)
    return rng.choice(pool, size=(outputs, terms))


PARITY = [("default", 256, 1), ("default", 1024, 3), ("default", 4096, 2), ("wide", 1024, 2), ("rns", 256, 1), ("rns", 4096, 2)]


@pytest.mark.parametrize("kind,n,k", PARITY)
def test_parity_with_lwe_linear_combine(pkg, kind, n, k):
    """every output row of both entry points equals the data of lwe_linear_combine on the same commitments and coefficient words, over
    the term counts around the recentring interval R, the output counts around the output tile T, shared terms, disjoint groups and a
    sliding window"""
    R, T = pkg._abi.COMBINE_TERMS, pkg._abi.COMBINE_OUTPUTS
    ctx = _ctx(pkg, kind, n, k)
    base, _ = _base(pkg, kind, n, k)
    rng = np.random.default_rng(n + k)
    term_counts, output_counts = [1, 2, R - 1, R, R + 1, 2 * R + 1], [1, T - 1, T, T + 1]
    index = np.arange(max(output_counts) * max(term_counts)) % BASE_ROWS
    rows = base[index]
    d_rows = _to_device(rows)
    cases = [(terms, outputs, stride) for terms in term_counts for outputs in output_counts for stride in (0, terms)] + [(R + 1, T + 1, 1)]
    for terms, outputs, stride in cases:
        coeffs = _draw(ctx, kind, rng, outputs, terms)
        got, status = _combine_device(ctx, d_rows, coeffs, stride)
        assert status.tolist() == [1] * outputs, (terms, outputs, stride)
        for j in range(outputs):
            want = _host_reference(pkg, (kind, n, k), ctx, base, index[j * stride:j * stride + terms], coeffs[j])
            assert want is not None and np.array_equal(got[j], want), (terms, outputs, stride, j)
        if outputs in (1, T + 1):                 # the flat twin on the same words (it stages through the device entry point)
            flat, flat_status = ctx.combine_rows(rows[:(outputs - 1) * stride + terms], coeffs, term_stride=stride)
            assert np.array_equal(flat, got) and np.array_equal(flat_status, status), (terms, outputs, stride)


def _synthetic_rows(ctx, header_row, rng):
    """three well-formed rows: every residue q - 1 (RNS: q_i - 1), all zero, uniformly random"""
    head, blocks = _layout(ctx)
    rows = np.repeat(header_row[None, :], 3, axis=0).copy()
    rows[:, head:] = 0
    for first, words, q in blocks:
        rows[0, first:first + words] = q - 1
        rows[2, first:first + words] = rng.integers(0, q, size=words, dtype=np.uint64)
    return rows


def test_exact_model_at_the_arithmetic_extreme(pkg):
    """Residues q - 1 under the largest multipliers: the accumulation bound of the FP64 kernel, pinned by big-integer arithmetic and not
    by the older kernel.  RNS: 100 terms with coefficients t/2 and t/2 + 1 (c' = t/2 and -(t/2)) alternating, all t/2, all t/2 + 1.
    Default: as many terms of +-1 as the budget admits."""
    rng = np.random.default_rng(2)
    rns = _ctx(pkg, "rns", 256, 1)
    t = rns.plain_modulus
    head, blocks = _layout(rns)
    three = _synthetic_rows(rns, _base(pkg, "rns", 256, 1)[0][0], rng)
    pick = np.zeros(100, dtype=np.int64)
    pick[[17, 63]], pick[[40, 99]] = 1, 2                     # the zero row and the random row among 96 rows of q - 1
    rows = three[pick]
    coeffs = np.array([[t // 2 + (i & 1) for i in range(100)], [t // 2] * 100, [t // 2 + 1] * 100, [t // 2 + 1 - (i & 1) for i in range(100)]], dtype=np.uint64)
    got, status = _both(rns, rows, coeffs, 0)
    assert status.tolist() == [1] * 4
    for j in range(4):
        assert got[j].tolist() == combine_model.combine_rows(rows, coeffs[j], t, head, blocks), j
    # default context: B terms of +-1 (exact in int64: B q < 2^57)
    ctx = _ctx(pkg, "default", 256, 1)
    t, q = ctx.plain_modulus, ctx.commit_modulus
    head, blocks = _layout(ctx)
    budget = _budget(pkg, ctx)
    three = _synthetic_rows(ctx, _base(pkg, "default", 256, 1)[0][0], rng)
    pick = np.zeros(budget, dtype=np.int64)
    pick[[5, budget // 2]], pick[[11, budget - 1]] = 1, 2
    rows = three[pick]
    signs = np.array([[1] * budget, [-1] * budget, [1 - 2 * (i & 1) for i in range(budget)]], dtype=np.int64)
    coeffs = np.where(signs > 0, np.uint64(1), np.uint64(t - 1)).astype(np.uint64)
    got, status = _both(ctx, rows, coeffs, 0)
    assert status.tolist() == [1] * 3
    body = rows[:, head:].astype(np.int64)
    for j in range(3):
        want = ((signs[j][:, None] * body).sum(axis=0) % q).astype(np.uint64)
        assert np.array_equal(got[j, :head], rows[0, :head]) and np.array_equal(got[j, head:], want), j


_BUDGETS = {}


def _budget(pkg, ctx):
    """the largest weight lwe_linear_combine accepts on this context, found by asking it with one large coefficient"""
    if ctx.handle not in _BUDGETS:
        t = ctx.plain_modulus
        row = _commit(ctx, np.zeros((1, 1), dtype=np.uint64), [3])[0]
        lo, hi = 1, t // 2                    # accepted, and (for a 44-bit context) refused
        assert _host_combine(pkg, ctx, [row], [lo]) is not None and _host_combine(pkg, ctx, [row], [hi]) is None
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if _host_combine(pkg, ctx, [row], [mid]) is not None:
                lo = mid
            else:
                hi = mid
        _BUDGETS[ctx.handle] = lo
    return _BUDGETS[ctx.handle]


def test_budget_boundary(pkg):
    ctx = _ctx(pkg, "default", 256, 1)
    base, _ = _base(pkg, "default", 256, 1)
    t = ctx.plain_modulus
    B = _budget(pkg, ctx)
    assert 2 < B < t // 2 - 1
    coeffs = np.array([[B - 1, 1], [B, 1], [t - (B - 1), t - 1]], dtype=np.uint64)          # weights B, B + 1, B (negative representatives)
    got, status = _both(ctx, base[:2], coeffs, 0)
    assert status.tolist() == [1, 0, 1]
    assert _host_combine(pkg, ctx, base[:2], coeffs[1]) is None and "noise budget" in pkg._abi.last_error()
    for j in (0, 2):
        assert np.array_equal(got[j], _host_combine(pkg, ctx, base[:2], coeffs[j])), j
    # the same boundary reached with all-ones coefficients over B and B + 1 terms
    index = np.arange(B + 1) % BASE_ROWS
    for terms, want in ((B, 1), (B + 1, 0)):
        got, status = _both(ctx, base[index[:terms]], np.ones((1, terms), dtype=np.uint64), 0)
        host = _host_combine(pkg, ctx, base[index[:terms]], [1] * terms)
        assert status.tolist() == [want] and (host is not None) == bool(want)
        if want:
            assert np.array_equal(got[0], host)
    # RNS: 64 coefficients of t/2 are far inside Q / 2t
    rns = _ctx(pkg, "rns", 256, 1)
    base, _ = _base(pkg, "rns", 256, 1)
    index = np.arange(64) % BASE_ROWS
    coeffs = np.full((1, 64), t // 2, dtype=np.uint64)
    got, status = _both(rns, base[index], coeffs, 0)
    assert status.tolist() == [1] and np.array_equal(got[0], _host_combine(pkg, rns, base[index], coeffs[0]))


@pytest.mark.parametrize("kind,n,k", PARITY)
def test_decoding_closes_the_loop(pkg, kind, n, k):
    """combined rows open to sum_i c'_i m_i mod t: lsr_lwe_decode_rows_device returns it and lsr_lwe_verify_rows_device accepts it"""
    import torch
    R, T = pkg._abi.COMBINE_TERMS, pkg._abi.COMBINE_OUTPUTS
    ctx = _ctx(pkg, kind, n, k)
    base, msgs = _base(pkg, kind, n, k)
    t = ctx.plain_modulus
    rng = np.random.default_rng(5 * n + k)
    terms, outputs = R + 1, T + 1
    for stride in (0, 3):
        index = np.arange((outputs - 1) * stride + terms) % BASE_ROWS
        coeffs = _draw(ctx, kind, rng, outputs, terms)
        got, status = _combine_device(ctx, _to_device(base[index]), coeffs, stride)
        assert status.tolist() == [1] * outputs
        want = np.array([[sum(combine_model.centred(int(c), t) * int(msgs[i, x]) for c, i in zip(coeffs[j], index[j * stride:j * stride + terms])) % t
                          for x in range(MSG_LEN)] for j in range(outputs)], dtype=np.uint64)
        decoded, decode_status = ctx.decode_rows(got, slots=MSG_LEN + 2)
        assert decode_status.tolist() == [1] * outputs
        assert np.array_equal(decoded[:, :MSG_LEN], want) and not decoded[:, MSG_LEN:].any()
        d_rows, d_msgs = _to_device(got), _to_device(want)
        d_res = torch.zeros(outputs, dtype=torch.int32, device="cuda")
        ctx.verify_rows_device(d_rows.data_ptr(), d_msgs.data_ptr(), MSG_LEN, outputs, d_res.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert d_res.cpu().tolist() == [1] * outputs


@pytest.mark.parametrize("kind,n,k", [("default", 256, 1), ("rns", 256, 1), ("wide", 1024, 2), ("default", 4096, 2)])
def test_malformed_terms(pkg, kind, n, k):
    """one bad term of output 2 in a call of four disjoint groups: status [1, 1, -1, 1], the three good rows as in the clean run,
    whether the bad term's coefficient is zero or not"""
    ctx = _ctx(pkg, kind, n, k)
    other_kind = "default" if kind == "rns" else "rns"
    other = _ctx(pkg, other_kind, n, k)
    base, _ = _base(pkg, kind, n, k)
    head, blocks = _layout(ctx)
    rng = np.random.default_rng(n + 11 * k)
    terms, outputs = 3, 4
    clean_rows = base[:terms * outputs].copy()
    victim = 2 * terms + 1
    foreign = np.zeros(ctx.commitment_words, dtype=np.uint64)
    row = _base(pkg, other_kind, n, k)[0][0]
    width = min(foreign.size, row.size)
    foreign[:width] = row[:width]                 # a row of the other kind of context, cut or padded to this row length

    def corrupted(edit):
        rows = clean_rows.copy()
        edit(rows[victim])
        return rows

    def set_word(w, value):
        def edit(r):
            r[w] = value
        return edit

    def set_row(r):
        r[:] = foreign

    variants = [set_word(1, int(clean_rows[victim, 1]) ^ 1), set_word(2, n | ((k + 1) << 32)), set_word(0, 8), set_row]
    for first, words, q in blocks:
        variants += [set_word(first, q), set_word(first + words - 1, q), set_word(first + words // 2 + 1, 2**64 - 1)]
    for zero_coefficient in (False, True):
        coeffs = _draw(ctx, kind, rng, outputs, terms)
        coeffs[2, 1] = 0 if zero_coefficient else 2
        clean, clean_status = _both(ctx, clean_rows, coeffs, terms)
        assert clean_status.tolist() == [1] * outputs
        for number, edit in enumerate(variants):
            got, status = _both(ctx, corrupted(edit), coeffs, terms)
            assert status.tolist() == [1, 1, -1, 1], (zero_coefficient, number)
            assert np.array_equal(got[[0, 1, 3]], clean[[0, 1, 3]]), (zero_coefficient, number)
    # shared terms: a bad term row spoils every output; a row width of the other kind of context is refused by the wrapper on the host
    rows = corrupted(variants[-1])[:victim + 1]
    _, status = _both(ctx, rows, _draw(ctx, kind, rng, 9, victim + 1), 0)
    assert status.tolist() == [-1] * 9
    with pytest.raises(ValueError):
        ctx.combine_rows(_base(pkg, other_kind, n, k)[0][:3], np.ones((1, 3), dtype=np.uint64))


def test_refusals(pkg, lib):
    import torch
    ctx = _ctx(pkg, "default", 256, 1)
    base, _ = _base(pkg, "default", 256, 1)
    W = ctx.commitment_words
    d_rows = _to_device(base[:4])
    d_coeffs = torch.ones(4, dtype=torch.int64, device="cuda")
    d_out = torch.full((2, W), -1, dtype=torch.int64, device="cuda")
    d_status = torch.full((2,), 77, dtype=torch.int32, device="cuda")
    h, s = ctx.handle, torch.cuda.current_stream().cuda_stream
    r, c, o, st = d_rows.data_ptr(), d_coeffs.data_ptr(), d_out.data_ptr(), d_status.data_ptr()
    h_rows, h_coeffs = np.ascontiguousarray(base[:4]), np.ones(4, dtype=np.uint64)
    h_out, h_status = np.full((2, W), 2**64 - 1, dtype=np.uint64), np.full(2, 77, dtype=np.int32)
    hr, hc, ho, hs = h_rows.ctypes.data, h_coeffs.ctypes.data, h_out.ctypes.data, h_status.ctypes.data
    dev, flat = lib.lsr_lwe_combine_rows_device, lib.lsr_lwe_combine_batch_flat
    refused = [
        (b"lsr_lwe_combine_rows_device", lambda: dev(None, r, 2, 2, c, 2, o, st, s)), (b"lsr_lwe_combine_rows_device", lambda: dev(h, None, 2, 2, c, 2, o, st, s)),
        (b"lsr_lwe_combine_rows_device", lambda: dev(h, r, 2, 2, None, 2, o, st, s)), (b"lsr_lwe_combine_rows_device", lambda: dev(h, r, 2, 2, c, 2, None, st, s)),
        (b"lsr_lwe_combine_rows_device", lambda: dev(h, r, 2, 2, c, 2, o, None, s)), (b"lsr_lwe_combine_rows_device", lambda: dev(h, r, 0, 2, c, 2, o, st, s)),
        (b"lsr_lwe_combine_rows_device", lambda: dev(h, r, 2, 2**63, c, 3, o, st, s)), (b"lsr_lwe_combine_rows_device", lambda: dev(h, r, 2, 2**61, c, 2, o, st, s)),
        (b"lsr_lwe_combine_rows_device", lambda: dev(h, r, 2**32, 0, c, 2, o, st, s)),
        (b"lsr_lwe_combine_batch_flat", lambda: flat(None, hr, 2, 2, hc, 2, ho, hs)), (b"lsr_lwe_combine_batch_flat", lambda: flat(h, None, 2, 2, hc, 2, ho, hs)),
        (b"lsr_lwe_combine_batch_flat", lambda: flat(h, hr, 2, 2, None, 2, ho, hs)), (b"lsr_lwe_combine_batch_flat", lambda: flat(h, hr, 2, 2, hc, 2, None, hs)),
        (b"lsr_lwe_combine_batch_flat", lambda: flat(h, hr, 2, 2, hc, 2, ho, None)), (b"lsr_lwe_combine_batch_flat", lambda: flat(h, hr, 0, 2, hc, 2, ho, hs)),
        (b"lsr_lwe_combine_batch_flat", lambda: flat(h, hr, 2, 2**63, hc, 3, ho, hs)), (b"lsr_lwe_combine_batch_flat", lambda: flat(h, hr, 2**32, 0, hc, 2, ho, hs)),
    ]
    for name, call in refused:
        assert not lib.lsr_lwe_context_create_rns(None, 3, -1) and b"NULL params" in lib.lsr_last_error()      # another text in between
        assert call() == -1
        assert name in lib.lsr_last_error() and b"NULL params" not in lib.lsr_last_error(), lib.lsr_last_error()
    assert dev(h, r, 2, 2, c, 0, o, st, s) == 0 and flat(h, hr, 2, 2, hc, 0, ho, hs) == 0
    torch.cuda.synchronize()
    assert d_status.cpu().tolist() == [77, 77] and bool((d_out == -1).all().item())                           # nothing was written
    assert h_status.tolist() == [77, 77] and bool((h_out == 2**64 - 1).all())


def test_combine_is_ordered_behind_a_commit_on_another_stream(pkg):
    """lsr_lwe_commit_rows_device on stream A, then lsr_lwe_combine_rows_device of those rows on stream B with no synchronisation by
    the caller: the context orders the two calls."""
    import torch
    n, k = 4096, 2
    ctx = _ctx(pkg, "default", n, k)
    rng = np.random.default_rng(13)
    batch, terms = 40, 4
    outputs = batch // terms
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    coeffs = _draw(ctx, "default", rng, outputs, terms)
    d_coeffs = _to_device(coeffs)
    for it in range(4):
        msgs = rng.integers(0, ctx.plain_modulus, size=(batch, MSG_LEN), dtype=np.uint64)
        keys = ctx.commit_keys(msgs, rng.integers(1, 2**63, size=batch, dtype=np.uint64))
        d_msgs, d_keys = _to_device(msgs), _to_device(keys)
        d_rows = torch.zeros((batch, ctx.commitment_words), dtype=torch.int64, device="cuda")
        d_out = torch.full((outputs, ctx.commitment_words), -1, dtype=torch.int64, device="cuda")
        d_status = torch.zeros(outputs, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.commit_rows_device(d_msgs.data_ptr(), MSG_LEN, batch, d_keys.data_ptr(), d_rows.data_ptr(), streams[0].cuda_stream)
        ctx.combine_rows_device(d_rows.data_ptr(), terms, d_coeffs.data_ptr(), outputs, d_out.data_ptr(), d_status.data_ptr(), term_stride=terms,
                                stream=streams[1].cuda_stream)
        torch.cuda.synchronize()
        assert d_status.cpu().tolist() == [1] * outputs, it
        rows, got = d_rows.cpu().numpy().view(np.uint64), d_out.cpu().numpy().view(np.uint64)
        for j in (0, outputs - 1):
            assert np.array_equal(got[j], _host_combine(pkg, ctx, rows[j * terms:(j + 1) * terms], coeffs[j])), (it, j)


def test_capture_into_a_graph_from_the_first_call(pkg):
    """One call captured on a FRESH context with no eager call before it, replayed with the coefficients and a term row changed between
    replays — over the budget and back, malformed and back: rows and status are right every time (the status is written by a kernel)."""
    import torch
    n, k = 256, 1
    ctx = pkg.LweContext(pkg.Params(n=n, k=k, sigma=SIGMA), key_seed=KEY)        # the keys of the cached context: its rows are rows of this one
    try:
        reference = _ctx(pkg, "default", n, k)
        base, _ = _base(pkg, "default", n, k)
        B = _budget(pkg, reference)
        t = ctx.plain_modulus
        terms, outputs = 5, 9
        rows = base[:terms].copy()
        d_rows = _to_device(rows)
        d_coeffs = torch.zeros((outputs, terms), dtype=torch.int64, device="cuda")
        d_out = torch.full((outputs, ctx.commitment_words), -1, dtype=torch.int64, device="cuda")
        d_status = torch.full((outputs,), 77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            ctx.combine_rows_device(d_rows.data_ptr(), terms, d_coeffs.data_ptr(), outputs, d_out.data_ptr(), d_status.data_ptr(), term_stride=0,
                                    stream=torch.cuda.current_stream().cuda_stream)
        rng = np.random.default_rng(21)
        small = _draw(ctx, "default", rng, outputs, terms)
        over = small.copy()
        over[4] = [B, 1, 0, 0, 0]                                              # weight B + 1
        again = _draw(ctx, "default", rng, outputs, terms)
        again[4] = [t - B, 0, 0, 0, 0]                                         # weight B, a negative representative
        broken = rows.copy()
        broken[3, 1] ^= 1
        plan = [(small, rows, [1] * outputs), (over, rows, [1, 1, 1, 1, 0, 1, 1, 1, 1]), (again, rows, [1] * outputs), (again, broken, [-1] * outputs),
                (small, rows[::-1].copy(), [1] * outputs)]
        for step, (coeffs, term_rows, want) in enumerate(plan):
            d_coeffs.copy_(_to_device(coeffs))
            d_rows.copy_(_to_device(term_rows))
            d_out.fill_(-1)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert d_status.cpu().tolist() == want, step
            got = d_out.cpu().numpy().view(np.uint64)
            for j in range(outputs):
                if want[j] == 1:
                    assert np.array_equal(got[j], _host_combine(pkg, reference, term_rows, coeffs[j])), (step, j)
    finally:
        ctx.close()


def test_flat_twin_spans_several_staging_chunks(pkg):
    """The flat verify exposes no knob for its staging chunk (about 1 GiB of rows and scratch per pass), so this call is large enough to
    span two passes at n = 256: shared terms and more outputs than one pass stages.  The coefficient vectors repeat with period 11, so
    the expected rows are those of an 11-output call, and the shared terms go up once."""
    ctx = _ctx(pkg, "default", 256, 1)
    base, _ = _base(pkg, "default", 256, 1)
    W, k, n = ctx.commitment_words, 1, 256
    per_pass = (1 << 30) // ((4 * k + 5) * n * 8)             # rows of one pass of the flat verify (lsr_commit.hip, verify_chunk)
    terms = 3
    outputs = per_pass - terms + 5                             # the first pass stages per_pass - terms outputs, the second the last 5
    rng = np.random.default_rng(8)
    few = _draw(ctx, "default", rng, 11, terms)
    few[7] = [_budget(pkg, ctx), 1, 0]                         # one vector over the budget: its status is 0 in both passes
    small, small_status = _both(ctx, base[:terms], few, 0)
    assert small_status.tolist() == [1] * 7 + [0] + [1] * 3
    pick = np.arange(outputs) % 11
    out, status = ctx.combine_rows(base[:terms], few[pick], term_stride=0)
    assert out.shape == (outputs, W) and np.array_equal(status, small_status[pick])
    good = status == 1
    assert np.array_equal(out[good], small[pick][good])
