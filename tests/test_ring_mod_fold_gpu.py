"""GPU suite: the fold of ring vectors by ring-valued challenges under an arbitrary modulus (RingMod.fold / fold_device,
lsr_ring_mod_fold_batch, batch.h "fold under any modulus").  Every output word and every status is compared exactly
with the Python-integer model (tests/ring_mod_fold_model.py: no primes, no groups), or — where the model would take more than
seconds — with RingMod.dot on the gathered operands, which the contract names as the definition.  Device outputs are one vector
longer than the call needs and come back with that tail untouched; out and status are pre-filled with sentinels."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import ring_mod_fold_model as fold_model
import ring_mod_model as model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P5 = model.prime_5_mod_8_below(1 << 32)
Q40 = fold_model.Q40
SENTINEL = 0x5A5A5A5A5A5A5A5A
STATUS_SENTINEL = 7


def _dev(torch, x):
    return torch.from_numpy(np.array(x, dtype=np.uint64, order="C").view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _vectors(outputs, terms, stride):
    return (outputs - 1) * stride + terms


def _device_fold(torch, ring, v, p, stride, bound_v=0, bound_p=0):
    """fold_device on copies of v [vectors, width, n] and p [outputs, terms, n]: (out, status), the guards checked"""
    outputs, terms, n = p.shape
    width = v.shape[1]
    d_v, d_p = _dev(torch, v), _dev(torch, p)
    d_out = torch.full((outputs + 1, width, n), SENTINEL, dtype=torch.int64, device="cuda")
    d_status = torch.full((outputs + 1,), STATUS_SENTINEL, dtype=torch.int32, device="cuda")
    ring.fold_device(d_out.data_ptr(), d_status.data_ptr(), d_v.data_ptr(), d_p.data_ptr(), outputs, terms, stride, width, bound_v, bound_p,
                     stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out, status = _host(d_out), d_status.cpu().numpy()
    assert bool((out[-1] == np.uint64(SENTINEL)).all()) and status[-1] == STATUS_SENTINEL, "the words behind out or status were written"
    return out[:-1], status[:-1]


def _model(v, p, q, stride, bound_v=0, bound_p=0):
    out, status = fold_model.fold(v.tolist(), p.tolist(), q, stride, bound_v, bound_p)
    return np.array(out, dtype=np.uint64).reshape(p.shape[0], v.shape[1], v.shape[2]), np.array(status, dtype=np.int32)


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def _gathered(ring, v, p, stride):
    """RingMod.dot on a[(j, c)][i] = v[j stride + i][c], b[(j, c)][i] = p[j][i]: the definition, on the device"""
    outputs, terms, n = p.shape
    width = v.shape[1]
    rows = np.arange(outputs)[:, None] * stride + np.arange(terms)[None, :]              # [outputs, terms]
    a = v[rows].transpose(0, 2, 1, 3).reshape(outputs * width, terms, n)                    # [outputs, width, terms, n]
    b = np.broadcast_to(p[:, None], (outputs, width, terms, n)).reshape(outputs * width, terms, n)
    return ring.dot(a, b).reshape(outputs, width, n)


def _short(rng, q, shape, bound):
    return (rng.integers(-bound, bound + 1, size=shape) % q).astype(np.uint64)


# ---- 1. model parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,q", [(2, 2), (4, 3329), (64, P5), (256, 3329), (64, 1 << 32)])
def test_model_parity_host_and_device_at_every_stride(pkg, n, q):
    """outputs 3, terms 3, width 3; shared, disjoint, overlapping and spaced terms; whole polynomials of floor(q/2) and floor(q/2) + 1"""
    import torch
    outputs = terms = width = 3
    h, hp = q // 2, min(q // 2 + 1, q - 1)
    rng = np.random.default_rng(n + q % 1000)
    with pkg.RingMod(q, n, device=0) as ring:
        for stride in (0, 3, 1, 4):
            v = model.planted(rng, q, (_vectors(outputs, terms, stride), width, n), {0: h, 1: hp, 2: h})
            p = model.planted(rng, q, (outputs, terms, n), {0: h, 1: h, 2: hp})
            want = _model(v, p, q, stride)
            assert want[1].tolist() == [1, 1, 1]
            assert _same(_device_fold(torch, ring, v, p, stride), want), (n, q, stride, "device")
            assert _same(ring.fold(v, p, stride), want), (n, q, stride, "host")
        out, status = ring.fold(v[:terms], p[0])                    # a 2-d p: one output
        assert status == 1 and np.array_equal(out, _model(v[:terms], p[:1], q, 0)[0][0])


# ---- 2. tiling ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,width", [(64, 65), (4096, 2)])
def test_full_and_ragged_tiles(pkg, n, width):
    """n = 64, width 65: 4160 words, one full tile and a ragged one holding a single component; n = 4096, width 2: two full tiles"""
    import torch
    q, outputs, terms = P5, 2, 2
    rng = np.random.default_rng(width)
    v, p = model.planted(rng, q, (terms + 1, width, n)), model.planted(rng, q, (outputs, terms, n))
    with pkg.RingMod(q, n, device=0) as ring:
        for stride in (0, 1):
            assert _same(_device_fold(torch, ring, v, p, stride), _model(v, p, q, stride)), (n, width, stride)


# ---- 3. every LT and both flavours -------------------------------------------------------------------------------------------------
def _sweep_width(logn):
    return 2 if logn == 12 else (4096 >> logn) + 3


@functools.lru_cache(maxsize=None)
def _sweep_reference(logn, name):
    """operands and the model's results of one (n, q): computed once, read-only, shared by the two flavours"""
    n = 1 << logn
    q = model.largest_admissible(n) if name == "top" else P5
    h, hp = q // 2, min(q // 2 + 1, q - 1)
    width = _sweep_width(logn)
    rng = np.random.default_rng(3500 + 100 * logn + (name == "top"))
    cases = []
    for outputs, terms, stride in [(2, 3, 1)] + ([(1, 33, 0)] if name == "P5" else []):
        # term 0 of output 0: all h by all h (+n h^2 at coefficient n - 1); of output 1: all h by all h + 1 (-n h^2)
        v = model.planted(rng, q, (_vectors(outputs, terms, stride), width, n), {0: h, 1: h})
        p = model.planted(rng, q, (outputs, terms, n), {0: h, 1: hp} if outputs > 1 else {0: h})
        want = _model(v, p, q, stride)
        for x in (v, p) + want:
            x.setflags(write=False)
        cases.append((v, p, stride, want))
    return q, cases


@pytest.mark.parametrize("logn", range(1, 13))
@pytest.mark.parametrize("name", ["top", "P5"])
@pytest.mark.parametrize("flavour", ["f64", "u64"])
def test_every_tile_size_flavour_and_modulus_edge(pkg, lib, flavour, name, logn):
    """width = 4096/n + 3 components (a full tile and a ragged one; 2 at n = 4096), 3 terms — under `top` (capacity 1) three groups,
    with n h^2 and -n h^2 at the ends of the CRT range — and under P5 also 33 terms, past the FP64 re-centring period"""
    import torch
    n = 1 << logn
    q, cases = _sweep_reference(logn, name)
    if name == "top":
        assert model.capacity(q, n) == 1 and fold_model.groups(q, n, 3) == [1, 1, 1]
    f64 = flavour == "f64"
    lib.lsr_set_arith_mode(0 if f64 else 1)
    try:
        ring = pkg.RingMod(q, n, device=0)
    finally:
        lib.lsr_set_arith_mode(0)
    with ring:
        assert ring.prime_context(0).uses_f64 == f64 == ring.prime_context(1).uses_f64
        for v, p, stride, want in cases:
            assert want[1].tolist() == [1] * p.shape[0]
            got = _device_fold(torch, ring, v, p, stride)
            assert _same(got, want), (flavour, name, n, p.shape[1])
        v, p, stride, want = cases[0]
        closed = n * (q // 2) ** 2 % q                            # coefficient n - 1 of all-h by all-h: no wrapped term there
        rest = sum(model.dot_coefficient([v[i, 0]], [p[0, i]], q, n - 1) for i in (1, 2))
        assert int(want[0][0, 0, n - 1]) == (closed + rest) % q


# ---- 4. grouping -------------------------------------------------------------------------------------------------------------------
def test_groups_of_terms_follow_the_declared_bounds(pkg):
    """q = 2^40 + 15, n = 64: 9 unbounded terms are groups of 7 + 2; the same operands with bound_p = 2 are one group; 16 terms with
    bound_p = floor(q/2) // 2 are groups of 15 + 1"""
    import torch
    q, n, width, outputs = Q40, 64, 2, 2
    h = q // 2
    assert fold_model.groups(q, n, 9) == [7, 2] and fold_model.groups(q, n, 9, 0, 2) == [9] and fold_model.groups(q, n, 16, 0, h // 2) == [15, 1]
    assert pkg.ring_mod_capacity_product(q, n, h, h) == 7 and pkg.ring_mod_capacity_product(q, n, h, 2) == 2199021131876
    assert pkg.ring_mod_capacity_product(q, n, h, h // 2) == 15
    rng = np.random.default_rng(4)
    with pkg.RingMod(q, n, device=0) as ring:
        v, p = model.planted(rng, q, (outputs * 9, width, n), {0: h, 9: h}), _short(rng, q, (outputs, 9, n), 2)
        want = _model(v, p, q, 9)
        assert want[1].tolist() == [1, 1]
        assert _same(_device_fold(torch, ring, v, p, 9), want), "7 + 2"
        assert _same(_device_fold(torch, ring, v, p, 9, 0, 2), want), "one group"
        assert _same(ring.fold(v, p, 9, 0, 2), want), "one group, host"
        v, p = model.planted(rng, q, (16 + 1, width, n), {0: h, 16: h}), _short(rng, q, (outputs, 16, n), h // 2)
        p[0, 0], p[1, 15] = h // 2, q - h // 2
        assert _same(_device_fold(torch, ring, v, p, 1, 0, h // 2), _model(v, p, q, 1, 0, h // 2)), "15 + 1"


# ---- 5. bounds ---------------------------------------------------------------------------------------------------------------------
def test_bounds_are_inclusive_and_gate_whole_outputs(pkg):
    import torch
    q, n, outputs, terms, width, bv, bp = 3329, 64, 3, 2, 2, 5, 2
    rng = np.random.default_rng(5)
    with pkg.RingMod(q, n, device=0) as ring:
        def run(v, p, stride, want_status):
            want = _model(v, p, q, stride, bv, bp)
            assert want[1].tolist() == want_status
            got = _device_fold(torch, ring, v, p, stride, bv, bp)
            assert _same(got, want), (stride, want_status, got[1])
            assert _same(ring.fold(v, p, stride, bv, bp), want), (stride, want_status, "host")
            for j, st in enumerate(want_status):
                assert bool(got[0][j].any()) == (st == 1)        # a gated output is all zero, its neighbours are not

        v, p = _short(rng, q, (outputs * terms, width, n), bv), _short(rng, q, (outputs, terms, n), bp)
        v[0, 0, 0], v[5, 1, n - 1], p[0, 0, 0], p[2, 1, n - 1] = bv, q - bv, bp, q - bp     # met exactly, from both sides
        run(v, p, terms, [1, 1, 1])
        for word in (bv + 1, q - bv - 1):                         # missed by one in v: output 1 reads vectors 2 and 3
            bad = v.copy()
            bad[3, 1, 7] = word
            run(bad, p, terms, [1, 0, 1])
        for word in (bp + 1, q - bp - 1):                         # missed by one in p
            bad = p.copy()
            bad[2, 0, n - 1] = word
            run(v, bad, terms, [1, 1, 0])
        bad_v, bad_p = v.copy(), p.copy()
        bad_v[0, 0, 1], bad_v[1, 1, 1] = bv + 1, q               # -1 wins over 0 within one output
        bad_p[2, 1, 0] = q + 1
        run(bad_v, bad_p, terms, [-1, 1, -1])
        bad_v[1, 1, 1] = 2**64 - 1
        run(bad_v, p, terms, [-1, 1, 1])
        # shared terms: a bad word of v gates every output, a bad word of p[j] gates j alone
        shared = v[:terms]
        bad = p.copy()
        bad[1, 1, 3] = bp + 1
        run(shared, bad, 0, [1, 0, 1])
        bad_v = shared.copy()
        bad_v[1, 0, 9] = q - bv - 1
        run(bad_v, p, 0, [0, 0, 0])
        bad[1, 1, 3] = q
        run(bad_v, bad, 0, [0, -1, 0])


def test_a_violation_in_the_last_group_zeroes_the_whole_output(pkg):
    """q = 2^40 + 15, n = 64, 9 unbounded terms (7 + 2): a word >= q in term 8 of v, then of p — the first group was reduced into out
    before the second found it"""
    import torch
    q, n, width, outputs, terms = Q40, 64, 2, 3, 9
    rng = np.random.default_rng(6)
    v, p = model.planted(rng, q, (outputs * terms, width, n)), model.planted(rng, q, (outputs, terms, n))
    with pkg.RingMod(q, n, device=0) as ring:
        assert fold_model.groups(q, n, terms) == [7, 2]
        bad = v.copy()
        bad[terms + 8, 1, n - 1] = q
        want = _model(bad, p, q, terms)
        assert want[1].tolist() == [1, -1, 1] and not want[0][1].any()
        assert _same(_device_fold(torch, ring, bad, p, terms), want)
        bad = p.copy()
        bad[2, 8, 0] = q
        assert _same(_device_fold(torch, ring, v, bad, terms), _model(v, bad, q, terms))
        # the same under a bound: bound_p = floor(q/2) - 1 still carries 7 products, and a challenge word of floor(q/2) misses it by one
        h = q // 2
        assert fold_model.groups(q, n, terms, 0, h - 1) == [7, 2]
        bad = _short(rng, q, p.shape, h - 1)
        bad[0, 8, n - 1] = h
        want = _model(v, bad, q, terms, 0, h - 1)
        assert want[1].tolist() == [0, 1, 1]
        assert _same(_device_fold(torch, ring, v, bad, terms, 0, h - 1), want)


# ---- 5b. operands and outputs off the vector alignment ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["top", "P5"])
@pytest.mark.parametrize("flavour", ["f64", "u64"])
def test_operands_and_outputs_off_the_vector_alignment(pkg, lib, flavour, name):
    """v, p and out start one word into their allocations: 8-byte but not 16-byte aligned, where the host takes the one-word-per-lane
    variants of the challenge lift and of the reduce (the tile kernel reads v where it lies).  n = 64, width 2, 3 outputs of 3 terms:
    under `top` with bound_p = floor(q/2) - 1 the capacity is 1, so every term is its own group — a plain and two accumulating
    reduces; under P5 with short operands the call is one group.  Output 1 holds a challenge word one over its bound and output 2 a
    word >= q, each in its LAST term: both come back as zeros, whatever the earlier groups wrote, by the one-word zero-fill.  The word
    before out, the word behind it and the words behind status stay as they were, and so do the operands."""
    import torch
    n, width, outputs, terms = 64, 2, 3, 3
    if name == "top":
        q = model.largest_admissible(n)
        bound_v, bound_p = 0, q // 2 - 1
        assert fold_model.groups(q, n, terms, bound_v, bound_p) == [1, 1, 1]
    else:
        q, bound_v, bound_p = P5, 1 << 20, 2
        assert fold_model.groups(q, n, terms, bound_v, bound_p) == [3]
    rng = np.random.default_rng(814 + (name == "top"))
    f64 = flavour == "f64"
    lib.lsr_set_arith_mode(0 if f64 else 1)
    try:
        ring = pkg.RingMod(q, n, device=0)
    finally:
        lib.lsr_set_arith_mode(0)

    def off_alignment(x):
        d = torch.full((x.size + 2,), SENTINEL, dtype=torch.int64, device="cuda")
        d[1:1 + x.size].copy_(_dev(torch, x).reshape(-1))
        assert (d.data_ptr() + 8) % 16 == 8
        return d

    def run(v, p, stride):
        d_v, d_p = off_alignment(v), off_alignment(p)
        words = outputs * width * n
        d_out = torch.full((words + 3,), SENTINEL, dtype=torch.int64, device="cuda")
        d_status = torch.full((outputs + 2,), STATUS_SENTINEL, dtype=torch.int32, device="cuda")
        assert (d_out.data_ptr() + 8) % 16 == 8
        ring.fold_device(d_out.data_ptr() + 8, d_status.data_ptr(), d_v.data_ptr() + 8, d_p.data_ptr() + 8, outputs, terms, stride, width, bound_v, bound_p,
                         stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        out, status = _host(d_out), d_status.cpu().numpy()
        assert out[0] == SENTINEL and (out[1 + words:] == SENTINEL).all(), "the words around out were written"
        assert status[outputs:].tolist() == [STATUS_SENTINEL] * 2, "the words behind status were written"
        for d, x in ((d_v, v), (d_p, p)):
            assert np.array_equal(_host(d)[1:-1], x.reshape(-1)) and _host(d)[0] == SENTINEL == _host(d)[-1], "an operand was written"
        return out[1:1 + words].reshape(outputs, width, n), status[:outputs]

    with ring:
        assert ring.prime_context(0).uses_f64 == f64 == ring.prime_context(1).uses_f64
        for stride in (terms, 0, 1):
            vectors = _vectors(outputs, terms, stride)
            v = _short(rng, q, (vectors, width, n), bound_v) if bound_v else model.planted(rng, q, (vectors, width, n), {0: q // 2})
            p = _short(rng, q, (outputs, terms, n), bound_p)
            p[0, 0, 0], p[2, terms - 1, n - 1] = bound_p, q - bound_p                     # the bound met from both sides
            want = _model(v, p, q, stride, bound_v, bound_p)
            assert want[1].tolist() == [1, 1, 1] and all(want[0][j].any() for j in range(outputs))
            assert _same(run(v, p, stride), want), (name, flavour, stride)
        # (stride 1) output 1: its last challenge one over the bound; output 2: a word >= q in the last vector it reads
        bad_v, bad_p = v.copy(), p.copy()
        bad_p[1, terms - 1, n - 1] = q - bound_p - 1
        bad_v[2 + terms - 1, width - 1, n - 1] = q
        want = _model(bad_v, bad_p, q, 1, bound_v, bound_p)
        got = run(bad_v, bad_p, 1)
        assert want[1].tolist() == [1, 0, -1] and _same(got, want), (name, flavour)
        assert got[0][0].any() and not got[0][1:].any()


# ---- 6. chunks ---------------------------------------------------------------------------------------------------------------------
def test_one_output_past_every_chunk_limit(pkg):
    """The limits of lsr_ring_mod_fold.hip, each crossed by one output or one component:
      sums         2^22 words per prime — n = 4096: 1024 polynomials.  width 5, terms 2, term_stride 0: 204 outputs fit (the challenge
                   rows would hold 256), outputs = 205.
      rows         min(4096, 2^21 / n) challenge transforms per prime — n = 2: 4096.  width 1, terms 1: 4096 outputs fit, outputs =
                   65537 is sixteen full chunks and one output.  (Grid y = 65535 is no limit of its own: a chunk never holds more
                   outputs than challenge rows, which a static_assert keeps below it; this shape would cross it if it were.)
      rows, terms  a chunk of fewer than 512 tiles keeps its outputs and shortens its groups instead — n = 4096: 512 rows.  width 1,
                   terms 3, outputs 300: 170 outputs would fit with whole sums; the call takes all 300 in three groups of one term,
                   and a word >= q in the last term still zeroes its output.
      wide output  an output of more than 2^22 / n components goes alone, its components in chunks, behind a check pass — n = 4096,
                   width 1025: one component past the first chunk; a word over the bound in that last component zeroes the output.
    The reference is RingMod.dot on the gathered operands."""
    import torch
    rng = np.random.default_rng(7)
    q, n = 1 << 32, 4096
    with pkg.RingMod(q, n, device=0) as ring:
        outputs, terms, width = 205, 2, 5
        v, p = rng.integers(0, q, size=(terms, width, n), dtype=np.uint64), rng.integers(0, q, size=(outputs, terms, n), dtype=np.uint64)
        p[204, 1, 4095] = q                                       # in the second chunk
        want = _gathered(ring, v, p, 0)
        want[204] = 0
        out, status = _device_fold(torch, ring, v, p, 0)
        assert status.tolist() == [1] * 204 + [-1] and np.array_equal(out, want)

        outputs, terms, width = 300, 3, 1
        v, p = rng.integers(0, q, size=(outputs + 2, width, n), dtype=np.uint64), rng.integers(0, q, size=(outputs, terms, n), dtype=np.uint64)
        v[171 + 2, 0, 0] = q                                      # term 2 of output 171 (its last group), term 1 of 172, term 0 of 173
        want = _gathered(ring, v, p, 1)
        want[171:174] = 0
        out, status = _device_fold(torch, ring, v, p, 1)
        assert status.tolist() == [1] * 171 + [-1] * 3 + [1] * 126 and np.array_equal(out, want)

        outputs, terms, width = 2, 1, 1025
        v, p = _short(rng, q, (2, width, n), 100), rng.integers(0, q, size=(outputs, terms, n), dtype=np.uint64)
        v[1, 1024, 17] = 101
        want = _gathered(ring, v, p, 1)
        want[1] = 0
        out, status = _device_fold(torch, ring, v, p, 1, 100, 0)
        assert status.tolist() == [1, 0] and np.array_equal(out, want)
    q, n, outputs = 3329, 2, 65537
    with pkg.RingMod(q, n, device=0) as ring:
        v, p = rng.integers(0, q, size=(outputs, 1, n), dtype=np.uint64), rng.integers(0, q, size=(outputs, 1, n), dtype=np.uint64)
        p[65536, 0, 1] = q
        want = _gathered(ring, v, p, 1)
        want[65536] = 0
        out, status = _device_fold(torch, ring, v, p, 1)
        assert status.tolist() == [1] * 65536 + [-1] and np.array_equal(out, want)


# ---- 7. host staging ---------------------------------------------------------------------------------------------------------------
_STAGED = dict(q=P5, n=64, outputs=40, terms=4, width=64, bound_v=1 << 20, bound_p=2)


def _staged_operands(stride):
    """n = 64, width 64, 4 terms, 40 outputs: under LAMBDA_SNARK_STAGING_MIB=1 (2048 polynomials per operand) 32, 8 or 29 outputs a chunk"""
    c = _STAGED
    rng = np.random.default_rng(70 + stride)
    v = _short(rng, c["q"], (_vectors(c["outputs"], c["terms"], stride), c["width"], c["n"]), c["bound_v"])
    p = _short(rng, c["q"], (c["outputs"], c["terms"], c["n"]), c["bound_p"])
    p[9, 1, 1], p[39, 3, 63] = 3, c["q"]
    if stride:
        v[0, 63, 63] = c["bound_v"] + 1                           # read by output 0 alone
    return v, p


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as entry
import test_ring_mod_fold_gpu as t
pkg, c, results = entry.load_package(), t._STAGED, {}
with pkg.RingMod(c["q"], c["n"], device=0) as ring:
    for stride in (0, 4, 1):
        v, p = t._staged_operands(stride)
        out, status = ring.fold(v, p, stride, c["bound_v"], c["bound_p"])
        results["out%d" % stride], results["status%d" % stride] = out, status
np.savez(sys.argv[2], **results)
"""


def test_plain_form_over_several_staged_chunks_equals_the_device_form(pkg, tmp_path):
    import torch
    assert "LAMBDA_SNARK_STAGING_MIB" not in os.environ
    script, out = tmp_path / "child.py", tmp_path / "out.npz"
    script.write_text(_CHILD)
    subprocess.run([sys.executable, str(script), ROOT, str(out)], check=True, env=dict(os.environ, LAMBDA_SNARK_STAGING_MIB="1"), timeout=300)
    got = np.load(str(out))
    c = _STAGED
    with pkg.RingMod(c["q"], c["n"], device=0) as ring:
        for stride in (0, 4, 1):
            v, p = _staged_operands(stride)
            want_out, want_status = _device_fold(torch, ring, v, p, stride, c["bound_v"], c["bound_p"])
            assert want_status.tolist().count(1) == (38 if stride == 0 else 37) and want_status[9] == 0 and want_status[39] == -1
            assert want_status[0] == (1 if stride == 0 else 0)
            assert np.array_equal(got["out%d" % stride], want_out) and np.array_equal(got["status%d" % stride], want_status), stride


# ---- 8. capture --------------------------------------------------------------------------------------------------------------------
def test_graph_capture_as_the_first_call_on_a_fresh_handle(pkg):
    """lsr_ring_mod_create allocated the workspace and there is no prepare: the capture is the handle's first call.  Groups of terms
    inside the graph (7 + 2); two replays on fresh inputs, the second with a word >= q."""
    import torch
    q, n, outputs, terms, width = Q40, 64, 2, 9, 3
    rng = np.random.default_rng(8)
    vectors = _vectors(outputs, terms, 1)
    d_v = torch.zeros((vectors, width, n), dtype=torch.int64, device="cuda")
    d_p = torch.zeros((outputs, terms, n), dtype=torch.int64, device="cuda")
    d_out = torch.full((outputs, width, n), SENTINEL, dtype=torch.int64, device="cuda")
    d_status = torch.full((outputs,), STATUS_SENTINEL, dtype=torch.int32, device="cuda")
    with pkg.RingMod(q, n, device=0) as ring, pkg.RingMod(q, n, device=0) as eager:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            ring.fold_device(d_out.data_ptr(), d_status.data_ptr(), d_v.data_ptr(), d_p.data_ptr(), outputs, terms, 1, width,
                             stream=torch.cuda.current_stream().cuda_stream)
        for replay in range(2):
            v, p = model.planted(rng, q, (vectors, width, n)), model.planted(rng, q, (outputs, terms, n))
            if replay == 1:
                v[vectors - 1, 2, 0] = q                          # the flags are cleared and set anew inside the graph
            d_v.copy_(_dev(torch, v))
            d_p.copy_(_dev(torch, p))
            graph.replay()
            torch.cuda.synchronize()
            got = (_host(d_out), d_status.cpu().numpy())
            assert _same(got, _device_fold(torch, eager, v, p, 1)) and _same(got, _model(v, p, q, 1))
            assert got[1].tolist() == ([1, 1] if replay == 0 else [1, -1])
