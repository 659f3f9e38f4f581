"""GPU suite: every instantiation of the ring-combine tile kernel, ring_combine_tile<A, LT> for LT = 1 .. 12 under both arithmetic
flavours, through lsr_lwe_ring_combine_rows_device and lsr_lwe_ring_combine_batch_flat.  The kernel's addressing is its own (the table of
outputs per tile polynomial, the (output, component, offset) of a tile index, the per-prime block offset, the one-polynomial-per-tile
path through buffer resources against the generic one, the two places a body word >= q lowers a status, the raw accumulator waiting in
the output row between groups of terms), so each LT is launched here in four kinds of context, each asserted to be what it claims:

    f64       the default 44-bit prime, FP64 arithmetic
    u64_q44   the same prime under lsr_set_arith_mode(1)
    u64_q60   the 60-bit prime of wide_modulus(n)
    rns       two 44-bit primes: two launches per call with different block offsets and header words

(An RNS context under arith mode 1 is left out: lsr_lwe_ntt_context refuses RNS contexts, so its flavour cannot be asserted.)

Every word is compared exactly with tests/ring_combine_model.py, which shares nothing with any kernel: the sparse form (exact integer
sums of shifted copies), for dense polynomials the schoolbook on Python integers at n <= 64 and the oracle's transforms above.  No
kernel result is compared with another kernel's; the host entry point is held against the device one only in addition."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ring_combine_model as model
import rns_model
from test_ring_combine_gpu import _sparse

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIGMA = 3.19
KEY = 77
K = 2                               # k + 1 = 3 components: with 4096/n polynomials per tile every tile boundary at n < 4096 splits an output
DEFAULT_Q = 17592169062401
SENTINEL = 0x5A5A5A5A5A5A5A5A
KINDS = ("f64", "u64_q44", "u64_q60", "rns")
CHUNK_MIB = 1                       # LAMBDA_SNARK_NTT_CHUNK_MIB of the child process of the groups-and-chunks test

_CONTEXTS = {}
_HEADERS = {}


def _ctx(pkg, lib, kind, n, k=K):
    """the context of this kind, once per module, asserted to run the arithmetic the kind names"""
    key = (kind, n, k)
    if key in _CONTEXTS:
        return _CONTEXTS[key]
    if kind == "rns":
        ctx = pkg.LweContext.create_rns(pkg.Params(n=n, k=k, sigma=SIGMA), key_seed=KEY)
    elif kind == "u64_q60":
        ctx = pkg.LweContext(pkg.Params(q=pkg.wide_modulus(n), n=n, k=k, sigma=SIGMA), key_seed=KEY)
    else:
        lib.lsr_set_arith_mode(1 if kind == "u64_q44" else 0)
        try:
            ctx = pkg.LweContext(pkg.Params(n=n, k=k, sigma=SIGMA), key_seed=KEY)
        finally:
            lib.lsr_set_arith_mode(0)
    _CONTEXTS[key] = ctx
    if kind == "rns":
        assert ctx.rns_moduli() == rns_model.rns_moduli(n), (kind, n)
    else:
        ntt = lib.lsr_lwe_ntt_context(ctx.handle)
        assert ntt, (kind, n)
        assert bool(lib.lsr_ntt_context_uses_f64(ntt)) == (kind == "f64"), (kind, n)
        assert ctx.rns_moduli() is None
        if n <= 4096:
            assert ctx.commit_modulus == (pkg.wide_modulus(n) if kind == "u64_q60" else DEFAULT_Q), (kind, n)
    assert (ctx.ring_degree, ctx.module_rank) == (n, k)
    return ctx


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for ctx in _CONTEXTS.values():
        ctx.close()
    _CONTEXTS.clear()
    _HEADERS.clear()


def _moduli(ctx):
    return tuple(ctx.rns_moduli() or (ctx.commit_modulus,))


def _genuine(pkg, ctx):
    """one committed row of the context: its header is the header of every term row"""
    if ctx.handle not in _HEADERS:
        n = ctx.ring_degree
        msgs = np.random.default_rng(n).integers(0, ctx.plain_modulus, size=(1, n), dtype=np.uint64)
        row = np.ascontiguousarray(pkg.Commitment.batch_words(ctx, msgs, np.array([5], dtype=np.uint64)), dtype=np.uint64)[0]
        assert row.size == ctx.commitment_words
        _HEADERS[ctx.handle] = row
    return _HEADERS[ctx.handle]


def _planted_words(q):
    return [0, 1, (q - 1) // 2, (q + 1) // 2, q - 1]


def _term_rows(rng, genuine, count, n, k, moduli):
    """count term rows: the genuine row first, then its header in front of uniformly random canonical residues per block, with the
    words 0, 1, (q - 1)/2, (q + 1)/2 and q - 1 at the first and last coefficient of the first and last component of every block.  (No
    commitment needs to be valid for this kernel.)"""
    head, blocks = model.layout(n, k, moduli)
    rows = np.zeros((count, genuine.size), dtype=np.uint64)
    assert genuine.size == head + len(moduli) * (k + 1) * n
    rows[:, :head] = genuine[:head]
    for first, words, q in blocks:
        rows[:, first:first + words] = rng.integers(0, q, size=(count, words), dtype=np.uint64)
        planted = np.array(_planted_words(q), dtype=np.uint64)
        for s, pos in enumerate((first, first + n - 1, first + k * n, first + words - 1)):
            rows[:, pos] = planted[(np.arange(count) + s) % 5]
    rows[0] = genuine
    return rows


def _polys(rng, kind, t, n, outputs, terms):
    """rns: dense polynomials of arbitrary 64-bit words with 0, 1, t - 1, (t -+ 1)/2, t + 5 and 2^64 - 1 at both ends.
    u64_q60: 2 - 4 taps out of (t - 1)/2, (t + 1)/2, t + 5 and 2^64 - 1, and one at each end of the first and the last polynomial.
    f64, u64_q44: the same taps out of +-1 and +-2 written as 1, 2, t - 1, t - 2, t + 1 and 3t + 1; output 0 gets one tap of
    (t - 1)/2 on top, which alone is over the budget of a 44-bit prime."""
    if kind == "rns":
        polys = rng.integers(0, 2**64, size=(outputs, terms, n), dtype=np.uint64)
        ends = np.array([0, 1, t - 1, (t - 1) // 2, (t + 1) // 2, t + 5, 2**64 - 1], dtype=np.uint64)
        which = np.arange(outputs)[:, None] + np.arange(terms)[None, :]
        polys[:, :, 0] = ends[which % 7]
        polys[:, :, n - 1] = ends[(which + 3) % 7]
        return polys
    small = kind != "u64_q60"
    pool = np.array([1, 2, t - 1, t - 2, t + 1, 3 * t + 1] if small else [(t - 1) // 2, (t + 1) // 2, t + 5, 2**64 - 1], dtype=np.uint64)
    polys = np.zeros((outputs, terms, n), dtype=np.uint64)
    for j in range(outputs):
        for i in range(terms):
            taps = rng.choice(n, size=min(n, int(rng.integers(2, 5))), replace=False)
            polys[j, i, taps] = rng.choice(pool, size=taps.size)
        polys[j, 0, n - 1], polys[j, terms - 1, 0] = rng.choice(pool, size=2)
    if small:
        polys[0, 1, n // 2] = (t - 1) // 2
    return polys


def _verdicts(ctx, polys):
    """the status the budget rule gives each output: 1 when its exact weight is within combine_max_weight"""
    return [1 if model.weight(p, ctx.plain_modulus) <= ctx.combine_max_weight else 0 for p in polys]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _device(ctx, rows, polys, term_stride):
    """the device entry point with one more output row (filled with a sentinel) and one more status (77) than the call has outputs:
    both must come back as they were -> (out rows, status)"""
    import torch
    outputs, terms = polys.shape[:2]
    d_rows, d_polys = _dev(rows), _dev(polys)
    d_out = torch.full((outputs + 1, ctx.commitment_words), SENTINEL, dtype=torch.int64, device="cuda")
    d_status = torch.full((outputs + 1,), 77, dtype=torch.int32, device="cuda")
    ctx.ring_combine_rows_device(d_rows.data_ptr(), terms, d_polys.data_ptr(), outputs, d_out.data_ptr(), d_status.data_ptr(), term_stride=term_stride,
                                 stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out, status = d_out.cpu().numpy().view(np.uint64), d_status.cpu().numpy()
    assert bool((out[-1] == np.uint64(SENTINEL)).all()), "the row behind the last output was written"
    assert status[-1] == 77, "the status behind the last output was written"
    return out[:-1], status[:-1]


def _both(ctx, rows, polys, term_stride):
    """the device entry point and the host one on the same inputs, asserted equal where the status is 1 -> (out rows, status)"""
    outputs, terms = polys.shape[:2]
    used = np.ascontiguousarray(rows[:(outputs - 1) * term_stride + terms])
    dev = _device(ctx, used, polys, term_stride)
    flat = ctx.ring_combine_rows(used, polys, term_stride=term_stride)
    assert np.array_equal(flat[1], dev[1])
    good = dev[1] == 1
    assert np.array_equal(flat[0][good], dev[0][good])
    return dev


def _outputs(logn):
    """ceil((P + 3)/3) + 1 outputs for P = 4096/n polynomials per tile: the 3 * outputs components fill one whole tile, go on into a
    ragged one and have an output on both sides of the boundary.  At n = 1024 that count makes exactly three whole tiles, so one more
    output is taken there and the last tile is ragged as everywhere else.  n = 4096: 2 outputs, one polynomial per tile."""
    if logn == 12:
        return 2
    per_tile = 4096 >> logn
    outputs = (per_tile + 3 + 2) // 3 + 1
    if (K + 1) * outputs % per_tile == 0:
        outputs += 1
    return outputs


def _reference(kind, n, oracle):
    """how the model multiplies: dense polynomials (rns) by the schoolbook at n <= 64 and through the oracle's transforms above, the
    sparse ones as sums of shifted copies"""
    if kind != "rns":
        return {}
    return {"schoolbook": True} if n <= 64 else {"oracle": oracle}


@pytest.mark.parametrize("logn", range(1, 13))
@pytest.mark.parametrize("kind", KINDS)
def test_every_kind_and_tile_size(pkg, lib, oracle, kind, logn):
    """3 terms per output, the outputs 4 term rows apart and once more over shared rows (term_stride = 0): the status of every output
    as the budget rule gives it, every word of every accepted output against the model, the row and the status behind the last output
    untouched, the host entry point equal to the device one; then the same call with one malformed body word."""
    n = 1 << logn
    ctx = _ctx(pkg, lib, kind, n)
    t, moduli, budget = ctx.plain_modulus, _moduli(ctx), ctx.combine_max_weight
    per_tile = 4096 >> logn
    outputs, terms = _outputs(logn), 3
    stride = terms + 1
    if logn < 12:
        assert (K + 1) * outputs > per_tile + K + 1 and (K + 1) * outputs % per_tile and per_tile % (K + 1)     # whole tile, ragged tile, split output
    rng = np.random.default_rng(1000 * logn + KINDS.index(kind))
    rows = _term_rows(rng, _genuine(pkg, ctx), (outputs - 1) * stride + terms, n, K, moduli)
    polys = _polys(rng, kind, t, n, outputs, terms)
    verdicts = _verdicts(ctx, polys)
    small = kind in ("f64", "u64_q44")
    assert not small or (t - 1) // 2 > budget
    assert verdicts == ([0] + [1] * (outputs - 1) if small else [1] * outputs), (budget, verdicts)
    good = np.array(verdicts) == 1
    ref = _reference(kind, n, oracle)
    clean = None
    for s in (stride, 0):
        got, status = _both(ctx, rows, polys, s)
        assert status.tolist() == verdicts, s
        want = model.combine_rows(rows, polys, s, t, n, K, moduli, **ref)
        assert np.array_equal(got[good], want[good]), (s, np.flatnonzero((got != want).any(axis=1)).tolist())
        clean = got if clean is None else clean

    # one body word of exactly q in the last block of a term row of the last output, in its last component: the ragged tile (n = 4096:
    # the second output).  Only that output's status drops, every other row is the clean run's.
    victim = outputs - 1
    last_first, last_words, last_q = model.layout(n, K, moduli)[1][-1]
    bad = rows.copy()
    bad[victim * stride + 1, last_first + K * n + n // 2] = last_q
    got, status = _both(ctx, bad, polys, stride)
    assert status.tolist() == verdicts[:victim] + [-1]
    assert np.array_equal(got[:victim][good[:victim]], clean[:victim][good[:victim]])


@pytest.mark.parametrize("logn", range(1, 13))
def test_recentring_period_at_every_tile_size(pkg, lib, oracle, logn):
    """FP64 with a large budget (rns): 33 and 65 identical term rows of all q - 1 against polynomials of all (t - 1)/2, so every
    product of one residue has one sign, across one and two re-centrings of the accumulator.  Both outputs have the same inputs, so
    the model is computed once."""
    assert pkg.RING_DOT_F64_RECENTRE_PERIOD == 32
    n = 1 << logn
    ctx = _ctx(pkg, lib, "rns", n)
    t, moduli, budget = ctx.plain_modulus, _moduli(ctx), ctx.combine_max_weight
    row = _genuine(pkg, ctx).copy()
    for first, words, q in model.layout(n, K, moduli)[1]:
        row[first:first + words] = q - 1
    ref = _reference("rns", n, oracle)
    for terms in (33, 65):
        rows = np.repeat(row[None, :], terms, axis=0)
        polys = np.full((2, terms, n), (t - 1) // 2, dtype=np.uint64)
        assert budget > 2**40 and terms * n * ((t - 1) // 2) == model.weight(polys[0], t) <= budget
        got, status = _both(ctx, rows, polys, 0)
        assert status.tolist() == [1, 1], terms
        want = model.combine_row(rows, polys[0], t, n, K, moduli, **ref)
        assert np.array_equal(got[0], want) and np.array_equal(got[1], want), terms


@pytest.mark.parametrize("logn", [14, 15, 17])
def test_composed_form_above_4096(pkg, lib, logn):
    """the composed form (unpack, lift, ring inner product) at the degrees between and above the suite's 8192 and 65536; n = 2^17
    goes through the ring inner product's two-pass form with a top round of 5 bits"""
    n, k = 1 << logn, 1
    ctx = _ctx(pkg, lib, "f64", n, k)
    t, moduli = ctx.plain_modulus, _moduli(ctx)
    rng = np.random.default_rng(logn)
    rows = _term_rows(rng, _genuine(pkg, ctx), 2, n, k, moduli)
    polys = _sparse(rng, ctx, 1, 2, n, every_word=False)
    assert _verdicts(ctx, polys) == [1]
    got, status = _both(ctx, rows, polys, 0)
    assert status.tolist() == [1]
    assert np.array_equal(got, model.combine_rows(rows, polys, 0, t, n, k, moduli))


_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as entry
pkg = entry.load_package()
data = np.load(sys.argv[2] + "/in.npz")
results, contexts = {}, {}
for name in str(data["names"]).split(","):
    kind, logn = name.split("-")[0], int(name.split("-")[1])
    n, k, stride = 1 << logn, int(data["k"]), int(data[name + "_stride"])
    if (kind, logn) not in contexts:
        if kind == "rns":
            contexts[kind, logn] = pkg.LweContext.create_rns(pkg.Params(n=n, k=k, sigma=float(data["sigma"])), key_seed=int(data["key"]))
        else:
            contexts[kind, logn] = pkg.LweContext(pkg.Params(q=pkg.wide_modulus(n), n=n, k=k, sigma=float(data["sigma"])), key_seed=int(data["key"]))
    ctx = contexts[kind, logn]
    polys = data[name + "_polys"]
    outputs, terms = polys.shape[:2]
    rows = data[name + "_rows"]
    rows = rows[np.arange((outputs - 1) * stride + terms) % rows.shape[0]]          # fewer distinct rows than terms: taken in turn
    d_rows = torch.from_numpy(rows.view(np.int64)).cuda()
    d_polys = torch.from_numpy(polys.view(np.int64)).cuda()
    d_out = torch.full((outputs, ctx.commitment_words), -1, dtype=torch.int64, device="cuda")
    d_status = torch.full((outputs,), 77, dtype=torch.int32, device="cuda")
    ctx.ring_combine_rows_device(d_rows.data_ptr(), terms, d_polys.data_ptr(), outputs, d_out.data_ptr(), d_status.data_ptr(), term_stride=stride,
                                 stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    results[name + "_out"] = d_out.cpu().numpy().view(np.uint64)
    results[name + "_status"] = d_status.cpu().numpy()
for ctx in contexts.values():
    ctx.close()
np.savez(sys.argv[2] + "/out.npz", **results)
"""


def _capacity(logn, rns):
    """ring_combine_polys of lsr_commit.hip at n <= 4096 under LAMBDA_SNARK_NTT_CHUNK_MIB = CHUNK_MIB: the polynomials per prime that
    one chunk of the workspace holds"""
    per_poly = (CHUNK_MIB << 20) >> (logn + 3)
    return max(1, per_poly // (2 if rns else 1))


def _few_taps(rng, t, outputs, terms, n):
    """two or three taps of +-1 per polynomial, written as 1, t - 1 and t + 1 (the third tap may fall on one of the first two and
    replace it)"""
    count = outputs * terms
    polys = np.zeros((count, n), dtype=np.uint64)
    words = np.array([1, t - 1, t + 1], dtype=np.uint64)
    first = rng.integers(0, n, size=count)
    for pos in (first, (first + rng.integers(1, n, size=count)) % n, rng.integers(0, n, size=count)):
        polys[np.arange(count), pos] = words[rng.integers(0, 3, size=count)]
    return polys.reshape(outputs, terms, n)


SHARED_ROWS = 7                     # distinct term rows of the many-term calls, taken in turn


@pytest.mark.parametrize("kind", ["rns", "u64_q60"])
def test_groups_of_terms_and_chunks_of_outputs_at_every_tile_size(pkg, lib, tmp_path, kind):
    """LAMBDA_SNARK_NTT_CHUNK_MIB=1 (read once per process: one fresh child per kind) leaves 2^(17 - LT) polynomials per prime to the
    workspace of a single-prime context and 2^(16 - LT) to an RNS one.  For rns (FP64) and u64_q60, at every LT = 4 .. 12:
      a) 2 outputs of capacity + 2 terms, one term row apart: one output per pass, its terms in two groups, the last of two terms,
         with the raw accumulator waiting in the output row in between.  The terms take 7 distinct rows in turn, so the model folds
         the polynomials that share a row (fold_shared_rows) and combines 7 terms;
      b) capacity/5 + 2 outputs of 5 terms: a full chunk of outputs and a ragged one.
    LT = 1 .. 3 would need 16386 to 65538 terms per output and are not run."""
    rng = np.random.default_rng(72 + len(kind))
    blob, want, names = {"sigma": SIGMA, "key": KEY, "k": K}, {}, []
    for logn in range(4, 13):
        n = 1 << logn
        ctx = _ctx(pkg, lib, kind, n)
        t, moduli, budget = ctx.plain_modulus, _moduli(ctx), ctx.combine_max_weight
        capacity = _capacity(logn, kind == "rns")
        assert capacity == 1 << ((16 if kind == "rns" else 17) - logn)
        genuine = _genuine(pkg, ctx)
        # a)
        name, outputs, terms, stride = "%s-%d-a" % (kind, logn), 2, capacity + 2, 1
        assert terms <= pkg._abi.RING_COMBINE_MAX_TERMS
        pool = _term_rows(rng, genuine, SHARED_ROWS, n, K, moduli)
        polys = _few_taps(rng, t, outputs, terms, n)
        assert all(int(np.abs(model.centred_words(p, t)).sum()) <= budget for p in polys)
        blob.update({name + "_stride": stride, name + "_rows": pool, name + "_polys": polys})
        want[name] = np.array([model.combine_row(pool, model.fold_shared_rows(polys[j], (j * stride + np.arange(terms)) % SHARED_ROWS, SHARED_ROWS, t),
                                                 t, n, K, moduli) for j in range(outputs)])
        names.append(name)
        # b)
        name, outputs, terms, stride = "%s-%d-b" % (kind, logn), capacity // 5 + 2, 5, 1
        assert capacity // 5 >= 1
        rows = _term_rows(rng, genuine, (outputs - 1) * stride + terms, n, K, moduli)
        polys = _few_taps(rng, t, outputs, terms, n)
        assert int(np.abs(model.centred_words(polys, t)).sum(axis=(1, 2)).max()) <= budget
        blob.update({name + "_stride": stride, name + "_rows": rows, name + "_polys": polys})
        want[name] = model.combine_rows(rows, polys, stride, t, n, K, moduli)
        names.append(name)
    blob["names"] = ",".join(names)
    np.savez(str(tmp_path / "in.npz"), **blob)
    script = tmp_path / "chunked.py"
    script.write_text(_CHILD)
    subprocess.run([sys.executable, str(script), ROOT, str(tmp_path)], check=True, env=dict(os.environ, LAMBDA_SNARK_NTT_CHUNK_MIB=str(CHUNK_MIB)), timeout=300)
    out = np.load(str(tmp_path / "out.npz"))
    for name in names:
        assert out[name + "_status"].tolist() == [1] * want[name].shape[0], name
        assert np.array_equal(out[name + "_out"], want[name]), name
