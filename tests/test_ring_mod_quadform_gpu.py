"""GPU suite: ring quadratic forms of a packed Gram triangle under an arbitrary modulus (RingMod.quadform* : lsr_ring_mod_quadform_*,
batch.h "quadratic forms under any modulus") against the Python-integer model (tests/ring_mod_quadform_model.py), the
composed public route and the verifier's identities on the handle.  Every comparison is exact, word for word, in both kernel flavours.
Shapes are the smallest at which each mechanism can fail: r in {1, 2, 5, 17} (one pair, one row piece, slices that start inside a
row), batch 3, the edge words of ring_mod_model in g and in c; 28 pairs against a capacity of 7 (groups of 3 and of 7 pairs reduced
with accumulate, driven to within a few bits of the CRT range); one family past the workspace at n = 65536; n = 8192 for the two-pass
transforms."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ring_mod_gram_model as gram_model
import ring_mod_model as mod
import ring_mod_quadform_model as model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P5 = 4294967197
Q40 = gram_model.Q40
BATCH = 3
FLAVOURS = ["f64", "u64"]
GROUP_BOUND_C = 1490944                     # q = P5, n = 64: capacity_quadform 7


def _dev(torch, x):
    return torch.from_numpy(np.array(x, dtype=np.uint64, order="C").view(np.int64)).cuda()          # (a copy: the references are read-only)


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _ring(pkg, q, n, flavour):
    """a handle whose prime contexts run the FP64 or the integer kernels (the switch is read when a context is created)"""
    lib = pkg._abi.lib()
    lib.lsr_set_arith_mode(0 if flavour == "f64" else 1)
    try:
        ring = pkg.RingMod(q, n, device=0)
    finally:
        lib.lsr_set_arith_mode(0)
    assert ring.prime_context(0).uses_f64 == (flavour == "f64") == ring.prime_context(1).uses_f64
    return ring


def _bounded(rng, q, shape, bound):
    """uniform centred words within `bound`, the bound met from both sides and 0, 1, q - 1 planted in the first polynomial"""
    v = rng.integers(-bound, bound + 1, size=shape, dtype=np.int64)
    x = np.where(v < 0, v + q, v).astype(np.uint64)
    first = x.reshape(-1, shape[-1])[0]
    for pos, word in zip(rng.choice(shape[-1], size=min(shape[-1], 5), replace=False).tolist(), [bound, q - bound, 0, 1, q - 1]):
        first[pos] = word
    return x


def _device(torch, ring, g, c, offdiag, bound_g=0, bound_c=0):
    """quadform_device on numpy operands (g [batch][pairs][n]; c [batch][r][n], or [r][n]: shared) -> (out, status); out and status are
    pre-filled, so what comes back was written, and g and c are checked to come back as they went"""
    batch, _, n = g.shape
    r = c.shape[-2]
    d_g, d_c = _dev(torch, g), _dev(torch, c)
    d_out = torch.full((batch, n), -1, dtype=torch.int64, device="cuda")
    d_status = torch.full((batch,), 7, dtype=torch.int32, device="cuda")
    ring.quadform_device(d_out.data_ptr(), d_status.data_ptr(), d_g.data_ptr(), d_c.data_ptr(), batch, r, 1 if c.ndim == 2 else batch, offdiag, bound_g, bound_c,
                         stream=_stream(torch))
    torch.cuda.synchronize()
    assert np.array_equal(_host(d_g), g) and np.array_equal(_host(d_c), c), "an operand was written"
    return _host(d_out), d_status.cpu().numpy()


def _want(g, c, q, offdiag, bound_g=0, bound_c=0):
    out, status = model.quadform(g.tolist(), [c.tolist()] if c.ndim == 2 else c.tolist(), q, offdiag, bound_g, bound_c)
    return np.array(out, dtype=np.uint64), np.array(status, dtype=np.int32)


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- 1. model parity ---------------------------------------------------------------------------------------------------------------
# (q, n, r, bound_c, offdiags): every q, n and r of the issue; bound_c = 2 where q >= 5; q = 3329 also unbounded, with (q + 1) / 2
PARITY = [
    (P5, 64, 17, 2, (1, 2, P5 - 1)),
    (P5, 2, 1, 2, (2,)),
    (1 << 32, 4096, 2, 2, (2, (1 << 32) - 1)),
    (1 << 32, 8192, 2, 2, (2,)),
    (Q40, 256, 5, 2, (1, 2, Q40 - 1)),
    (Q40, 4, 5, 2, (2,)),
    (3329, 256, 5, 2, (1, 2, 3328)),
    (3329, 256, 2, 0, (2, (3329 + 1) // 2)),
    (3, 4, 2, 0, (1, 2)),
    (3, 64, 5, 0, (2,)),
    (2, 2, 1, 0, (1,)),
    (2, 64, 5, 0, (1,)),
]


@functools.lru_cache(maxsize=None)
def _parity_reference(q, n, r, bound_c, offdiags):
    rng = np.random.default_rng(3700 * n + q % 991 + r)
    pairs = r * (r + 1) // 2
    g = mod.planted(rng, q, (BATCH, pairs, n))
    c = _bounded(rng, q, (BATCH, r, n), bound_c) if bound_c else mod.planted(rng, q, (BATCH, r, n))
    want = {(w, shared): _want(g, c[1] if shared else c, q, w, 0, bound_c) for w in offdiags for shared in (False, True)}
    for arr in (g, c) + tuple(v[0] for v in want.values()):
        arr.setflags(write=False)
    return g, c, want


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("q,n,r,bound_c,offdiags", PARITY)
def test_quadform_equals_the_model_word_for_word(pkg, q, n, r, bound_c, offdiags, flavour):
    import torch
    g, c, want = _parity_reference(q, n, r, bound_c, offdiags)
    assert model.groups(q, n, r, max(offdiags, key=lambda w: model.weight(q, w)), 0, bound_c) == [r * (r + 1) // 2]      # one group: it fits
    ones = np.ones(BATCH, dtype=np.int32)
    with _ring(pkg, q, n, flavour) as ring:
        for (w, shared), ref in want.items():
            cc = c[1] if shared else c
            got = _device(torch, ring, g, cc, w, 0, bound_c)
            assert _same(got, ref) and np.array_equal(got[1], ones), (w, shared)
        w = offdiags[-1]
        assert _same(ring.quadform(g, c, w, 0, bound_c), want[(w, False)])                    # the host forms
        assert _same(ring.quadform(g, c[1], w, 0, bound_c), want[(w, True)])
        out1, st1 = ring.quadform(g[2], c[2], w, 0, bound_c)                                    # 2-d operands: a batch of one
        assert np.array_equal(out1, want[(w, False)][0][2]) and st1 == 1


def test_capacity_at_3329_holds_the_weight_of_the_half(pkg):
    q = 3329
    assert pkg.ring_mod_capacity_quadform(q, 256, 0, 0) == 512471014808 and model.weight(q, (q + 1) // 2) == 1664


# ---- 2. the composed public route ---------------------------------------------------------------------------------------------------
def test_quadform_equals_mul_per_pair_a_scaling_and_dot(pkg):
    q, n, r, offdiag = 3329, 256, 5, 2
    g, c, want = _parity_reference(q, n, r, 2, (1, 2, 3328))
    order = [(i, l) for i in range(r) for l in range(i, r)]
    scale = np.array([1 if i == l else offdiag for i, l in order], dtype=np.uint64)[:, None]
    with pkg.RingMod(q, n, device=0) as ring:
        for j in range(BATCH):
            products = ring.mul(c[j][[i for i, _ in order]], c[j][[l for _, l in order]])
            composed = ring.dot(g[j], products * scale % np.uint64(q))
            assert np.array_equal(composed, want[(offdiag, False)][0][j]), j
        assert _same(ring.quadform(g, c, offdiag, 0, 2), want[(offdiag, False)])


# ---- 3. capacity groups -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _grouped_operands():
    """q = P5, n = 64, r = 7 (28 pairs), challenges within 1490944: P carries 7 triple products.  Families 0 and 1 are random with the
    bounds met; family 2 is the extreme: every c_i = bound_c (1 + X + ... + X^(n - 1)) and every g word +-floor(q / 2), signed so that
    coefficient n - 1 of every triple product is n^2 floor(q / 2) bound_c^2 / 2."""
    q, n, r = P5, 64, 7
    h = q // 2
    rng = np.random.default_rng(1490944)
    g = mod.planted(rng, q, (BATCH, 28, n))
    c = _bounded(rng, q, (BATCH, r, n), GROUP_BOUND_C)
    c[2] = GROUP_BOUND_C
    g[2] = np.array([h if 2 * (n - 1 - a) + 2 - n > 0 else q - h for a in range(n)], dtype=np.uint64)
    g.setflags(write=False)
    c.setflags(write=False)
    return g, c


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("offdiag,size", [(2, 3), (1, 7)])
def test_pair_groups_follow_the_capacity_up_to_the_crt_range(pkg, offdiag, size, flavour):
    import torch
    q, n, r = P5, 64, 7
    g, c = _grouped_operands()
    # the group rule, restated: floor(capacity / max(1, |centred offdiag|)) pairs a group, in runs of the packed order
    capacity = pkg.ring_mod_capacity_quadform(q, n, 0, GROUP_BOUND_C)
    assert capacity == 7 == model.capacity_quadform(q, n, 0, GROUP_BOUND_C)
    per = capacity // max(1, min(offdiag, q - offdiag))
    sizes = [min(per, 28 - p0) for p0 in range(0, 28, per)]
    assert per == size and sizes == model.groups(q, n, r, offdiag, 0, GROUP_BOUND_C) and len(sizes) > 1
    # the extreme family drives some group's integer to within a few bits of the CRT range, and none beyond it
    p1, p2 = mod.primes(n)
    half_p = (p1 * p2 - 1) // 2
    magnitudes = model.group_magnitudes(g[2].tolist(), c[2].tolist(), q, offdiag, sizes)
    assert half_p // 16 < max(magnitudes) <= half_p, (max(magnitudes) / half_p)
    want = _want(g, c, q, offdiag, 0, GROUP_BOUND_C)
    shared = _want(g, c[2], q, offdiag, 0, GROUP_BOUND_C)
    assert want[1].tolist() == [1, 1, 1] and want[0].any()
    with _ring(pkg, q, n, flavour) as ring:
        assert _same(_device(torch, ring, g, c, offdiag, 0, GROUP_BOUND_C), want)
        assert _same(_device(torch, ring, g, c[2], offdiag, 0, GROUP_BOUND_C), shared)
        assert _same(ring.quadform(g, c, offdiag, 0, GROUP_BOUND_C), want)


# ---- 4. workspace groups ------------------------------------------------------------------------------------------------------------
def _workspace_words():
    """per prime, as batch.h states it"""
    text = open(os.path.join(ROOT, "include", "lambda_snark", "batch.h")).read()
    m = re.search(r"per prime max\(2\^(\d+), LAMBDA_SNARK_NTT_CHUNK_MIB 2\^20 / (\d+)\)", text)
    assert m, "batch.h states the size of the Gram workspace"
    chunk_mib = int(os.environ.get("LAMBDA_SNARK_NTT_CHUNK_MIB", "0") or 0)
    return max(1 << int(m.group(1)), (chunk_mib if chunk_mib > 0 else 256) * (1 << 20) // int(m.group(2)))


@functools.lru_cache(maxsize=None)
def _monomial_reference():
    """n = 65536, q = 2^32, r = 16, batch 2: the challenges are signed monomials s_i X^(e_i), so a triple product is a signed negacyclic
    rotation of g_il by e_i + e_l — exact in numpy, where sums wrap at 2^64, a multiple of q"""
    q, n, r, batch, offdiag = 1 << 32, 65536, 16, 2, 2
    rng = np.random.default_rng(65536)
    g = rng.integers(0, q, size=(batch, r * (r + 1) // 2, n), dtype=np.uint64)
    exps, signs = rng.integers(0, n, size=(batch, r)), rng.choice([1, -1], size=(batch, r))
    c = np.zeros((batch, r, n), dtype=np.uint64)
    for j in range(batch):
        for i in range(r):
            c[j, i, exps[j, i]] = 1 if signs[j, i] > 0 else q - 1
    want = np.zeros((batch, n), dtype=np.uint64)
    for j in range(batch):
        for i in range(r):
            for l in range(i, r):
                k, sign = int(exps[j, i] + exps[j, l]), int(signs[j, i] * signs[j, l])
                if k >= n:
                    k, sign = k - n, -sign
                poly = g[j, gram_model.index(r, i, l)]
                rotated = np.concatenate([np.uint64(0) - poly[n - k:], poly[:n - k]]) if k else poly
                term = rotated * np.uint64(1 if i == l else offdiag)
                want[j] = want[j] + term if sign > 0 else want[j] - term
    want &= np.uint64(q - 1)
    for arr in (g, c, want):
        arr.setflags(write=False)
    return g, c, want, offdiag


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_one_family_past_the_workspace_takes_pair_groups(pkg, flavour):
    import torch
    q, n, r = 1 << 32, 65536, 16
    pairs, polys = r * (r + 1) // 2, _workspace_words() // n
    # the documented plan: a chunk holds, per prime, a family's r transformed challenges, its group of g and one sum
    assert pairs * n > _workspace_words() and r + pairs + 1 > polys >= r + 3
    assert pkg.ring_mod_capacity_quadform(q, n, 0, 1) >= 2 * pairs                    # the capacity does not cut: the workspace does
    g, c, want, offdiag = _monomial_reference()
    with _ring(pkg, q, n, flavour) as ring:
        got = _device(torch, ring, g, c, offdiag, 0, 1)
        assert got[1].tolist() == [1, 1] and np.array_equal(got[0], want)


# ---- 5. status ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_bounds_are_verified_per_family_across_groups(pkg, flavour):
    """the 28-pair shape in groups of 3 pairs, bound_g = floor(q / 2) - 1: every offending word of g sits in the last group's last pair,
    so the outputs the earlier groups wrote are zeroed all the same"""
    import torch
    q, n, r, offdiag = P5, 64, 7, 2
    h = q // 2
    bound_g, bound_c = h - 1, GROUP_BOUND_C
    assert model.groups(q, n, r, offdiag, bound_g, bound_c) == [3] * 9 + [1]
    rng = np.random.default_rng(28)
    clean_g = _bounded(rng, q, (4, 28, n), bound_g)
    clean_c = _bounded(rng, q, (4, r, n), bound_c)
    clean = _want(clean_g, clean_c, q, offdiag, bound_g, bound_c)
    assert clean[1].tolist() == [1, 1, 1, 1] and all(clean[0][j].any() for j in range(4))

    def planted(words_g, words_c):
        g, c = clean_g.copy(), clean_c.copy()
        for (j, pos), word in words_g.items():
            g[j, 27, pos] = word
        for (j, i, pos), word in words_c.items():
            c[j, i, pos] = word
        return g, c

    with _ring(pkg, q, n, flavour) as ring:
        assert _same(_device(torch, ring, clean_g, clean_c, offdiag, bound_g, bound_c), clean)
        cases = [
            # over bound_g (+h and -h) in the last pair; over bound_c; a word >= q in g
            (planted({(1, n - 1): h, (3, 0): q}, {(2, r - 1, 5): bound_c + 1}), [1, 0, 0, -1]),
            (planted({(0, 3): h + 1}, {(2, 0, 0): q - bound_c - 1}), [0, 1, 0, 1]),
            # a word >= q in c; an over-bound word and a word >= q in one family: -1 wins, whichever operand holds which
            (planted({(2, 7): h, (3, 9): q + 5}, {(1, 3, n - 1): q, (2, 1, 1): 2**64 - 1, (3, 0, 0): bound_c + 1}), [1, -1, -1, -1]),
        ]
        for (g, c), statuses in cases:
            want = _want(g, c, q, offdiag, bound_g, bound_c)
            assert want[1].tolist() == statuses
            for got in (_device(torch, ring, g, c, offdiag, bound_g, bound_c), ring.quadform(g, c, offdiag, bound_g, bound_c)):
                assert _same(got, want)
                for j, st in enumerate(statuses):                       # gated outputs are all zero, the others untouched
                    assert np.array_equal(got[0][j], clean[0][j]) if st == 1 else not got[0][j].any(), j
        # a shared c: a bad word gates every family, a bad word of g its own family alone
        shared = clean_c[0].copy()
        ok = _want(clean_g, shared, q, offdiag, bound_g, bound_c)
        assert ok[1].tolist() == [1, 1, 1, 1] and _same(_device(torch, ring, clean_g, shared, offdiag, bound_g, bound_c), ok)
        g, _ = planted({(2, 1): h}, {})
        got = _device(torch, ring, g, shared, offdiag, bound_g, bound_c)
        assert got[1].tolist() == [1, 1, 0, 1] and _same(got, _want(g, shared, q, offdiag, bound_g, bound_c))
        shared[r - 1, n - 1] = bound_c + 1
        for got in (_device(torch, ring, clean_g, shared, offdiag, bound_g, bound_c), ring.quadform(clean_g, shared, offdiag, bound_g, bound_c)):
            assert got[1].tolist() == [0, 0, 0, 0] and not got[0].any()
        shared[0, 0] = q
        got = _device(torch, ring, clean_g, shared, offdiag, bound_g, bound_c)
        assert got[1].tolist() == [-1, -1, -1, -1] and not got[0].any()
        # and the flags are set anew by the next call
        assert _same(_device(torch, ring, clean_g, clean_c, offdiag, bound_g, bound_c), clean)


# ---- 5b. operands and outputs off the vector alignment ---------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_operands_and_outputs_off_the_vector_alignment(pkg, flavour):
    """g, c and out start one word into their allocations: 8-byte but not 16-byte aligned, where the host takes the one-word-per-lane
    variants of the lift and of the reduce.  28 pairs against a capacity of 7 are four groups: a check of the whole g without stores,
    lifts of g without the check, a plain and three accumulating reduces; r = 2 is one group, the check riding in the lift.  Family 1
    holds a word over bound_g in its last pair, family 2 a word >= q: both come back as zeros, whatever the earlier groups wrote, by
    the one-word zero-fill.  The word before out, the word behind it and the words behind status stay as they were, and so do the
    operands."""
    import torch
    q, n, r, batch = P5, 64, 7, 4
    h = q // 2
    bound_g, bound_c = h - 1, GROUP_BOUND_C
    sentinel, status_sentinel = 0x5A5A5A5A5A5A5A5A, 7
    assert model.groups(q, n, r, 1, bound_g, bound_c) == [7, 7, 7, 7] and model.groups(q, n, 2, 2, bound_g, bound_c) == [3]
    rng = np.random.default_rng(815)

    def off_alignment(x):
        d = torch.full((x.size + 2,), sentinel, dtype=torch.int64, device="cuda")
        d[1:1 + x.size].copy_(_dev(torch, x).reshape(-1))
        assert (d.data_ptr() + 8) % 16 == 8
        return d

    def run(ring, g, c, offdiag):
        d_g, d_c = off_alignment(g), off_alignment(c)
        d_out = torch.full((batch * n + 3,), sentinel, dtype=torch.int64, device="cuda")
        d_status = torch.full((batch + 2,), status_sentinel, dtype=torch.int32, device="cuda")
        assert (d_out.data_ptr() + 8) % 16 == 8
        ring.quadform_device(d_out.data_ptr() + 8, d_status.data_ptr(), d_g.data_ptr() + 8, d_c.data_ptr() + 8, batch, c.shape[-2],
                             1 if c.ndim == 2 else batch, offdiag, bound_g, bound_c, stream=_stream(torch))
        torch.cuda.synchronize()
        out, status = _host(d_out), d_status.cpu().numpy()
        assert out[0] == sentinel and (out[1 + batch * n:] == sentinel).all(), "the words around out were written"
        assert status[batch:].tolist() == [status_sentinel] * 2, "the words behind status were written"
        for d, x in ((d_g, g), (d_c, c)):
            assert np.array_equal(_host(d)[1:-1], x.reshape(-1)) and _host(d)[0] == sentinel == _host(d)[-1], "an operand was written"
        return out[1:1 + batch * n].reshape(batch, n), status[:batch]

    def check(ring, g, c, offdiag, statuses):
        want = _want(g, c, q, offdiag, bound_g, bound_c)
        assert want[1].tolist() == statuses
        got = run(ring, g, c, offdiag)
        assert _same(got, want)
        for j, st in enumerate(statuses):
            assert bool(got[0][j].any()) == (st == 1), j

    with _ring(pkg, q, n, flavour) as ring:
        g, c = _bounded(rng, q, (batch, 28, n), bound_g), _bounded(rng, q, (batch, r, n), bound_c)
        check(ring, g, c, 1, [1, 1, 1, 1])
        check(ring, g, c[0], 1, [1, 1, 1, 1])                                   # a shared c
        bad_g, bad_c = g.copy(), c.copy()
        bad_g[1, 27, n - 1], bad_c[2, r - 1, 0] = h, q                          # the last group's last pair; a challenge word >= q
        check(ring, bad_g, bad_c, 1, [1, 0, -1, 1])
        bad_g[2, 27, 0] = q + 5
        check(ring, bad_g, c[0], 1, [1, 0, -1, 1])                              # a shared c: the families' own g words
        shared = c[0].copy()
        shared[r - 1, n - 1] = bound_c + 1                                      # ... and a shared word over its bound gates them all
        check(ring, g, shared, 1, [0, 0, 0, 0])
        # r = 2 with offdiag 2: three pairs in one group
        g2, c2 = _bounded(rng, q, (batch, 3, n), bound_g), _bounded(rng, q, (batch, 2, n), bound_c)
        check(ring, g2, c2, 2, [1, 1, 1, 1])
        g2[3, 2, n - 1], c2[0, 0, n - 1] = q - h, 2**64 - 1
        check(ring, g2, c2, 2, [-1, 1, 1, 0])


# ---- 6. refusals that read the handle -----------------------------------------------------------------------------------------------
def test_refusals_on_a_real_handle(pkg):
    import torch
    q, n, r = P5, 64, 2
    d = [torch.zeros((2, 3, n), dtype=torch.int64, device="cuda") for _ in range(3)]
    d_status = torch.zeros(2, dtype=torch.int32, device="cuda")
    out, g, c, st = d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d_status.data_ptr()
    with pkg.RingMod(q, n, device=0) as ring:
        lib, name = ring._lib, "lsr_ring_mod_quadform_batch_device"

        def refused(word, *args):
            assert lib.lsr_ring_mod_quadform_batch_device(ring.handle, *args, None) == -1
            msg = pkg._abi.last_error()
            assert msg.startswith(name + ":") and word in msg, msg
            return msg

        # the capacity: unbounded challenges — the message names bound_c and the route that always works — before the overlap
        msg = refused("bound_c", g, st, g, c, 2, r, 2, 2, 0, 0)
        assert "lsr_ring_mod_mul_batch" in msg and "lsr_ring_mod_dot_batch" in msg
        with pytest.raises(pkg.CoreError, match="bound_c"):
            ring.quadform(np.zeros((3, n), dtype=np.uint64), np.zeros((2, n), dtype=np.uint64))
        refused("offdiag", g, st, g, c, 2, r, 2, q, 0, 2)
        refused("out overlaps g", g, st, g, c, 2, r, 2, 2, 0, 2)
        refused("out overlaps c", c + 8, st, g, c, 2, r, 2, 2, 0, 2)
        refused("status overlaps g", out, g + 16, g, c, 2, r, 2, 2, 0, 2)
        refused("status overlaps out", out, out, g, c, 2, r, 2, 2, 0, 2)
        assert lib.lsr_ring_mod_quadform_batch_device(ring.handle, g, st, g, c, 0, r, 1, 2, 0, 2, None) == 0          # the empty call
        assert lib.lsr_ring_mod_quadform_batch_device(ring.handle, out, st, g, c, 2, r, 2, 2, 0, 2, None) == 0
        torch.cuda.synchronize()
        assert d_status.tolist() == [1, 1]


def test_capture_without_the_workspace_is_refused_and_leaves_the_handle_usable(pkg):
    import torch
    q, n, r = 3329, 256, 5
    g, c, want = _parity_reference(q, n, r, 2, (1, 2, 3328))
    d_g, d_c = _dev(torch, g), _dev(torch, c)
    d_out = torch.zeros((BATCH, n), dtype=torch.int64, device="cuda")
    d_status = torch.zeros(BATCH, dtype=torch.int32, device="cuda")
    with pkg.RingMod(q, n, device=0) as ring:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            d_out.add_(0)                  # (keeps the captured graph non-empty)
            rc = ring._lib.lsr_ring_mod_quadform_batch_device(ring.handle, d_out.data_ptr(), d_status.data_ptr(), d_g.data_ptr(), d_c.data_ptr(), BATCH, r, BATCH,
                                                              2, 0, 2, torch.cuda.current_stream().cuda_stream)
        assert rc == -1
        msg = pkg._abi.last_error()
        assert msg.startswith("lsr_ring_mod_quadform_batch_device:") and "workspace" in msg and "eager" in msg
        graph.replay()                     # the capture stayed usable
        torch.cuda.synchronize()
        assert not bool(d_out.any())       # and holds no launch of the refused call
        assert _same(_device(torch, ring, g, c, 2, 0, 2), want[(2, False)])


# ---- 7. capture -----------------------------------------------------------------------------------------------------------------------
def test_graph_capture_after_prepare(pkg):
    """no eager call first: gram_prepare allocated the workspace.  Pair groups inside the graph, which is one chain on a side stream;
    two replays on fresh inputs, each equal to the eager call on the same inputs."""
    import torch
    q, n, r, offdiag, batch = P5, 64, 7, 2, BATCH
    base_g, base_c = _grouped_operands()
    ring = pkg.RingMod(q, n, device=0)
    ring.gram_prepare()
    d_g = torch.zeros((batch, 28, n), dtype=torch.int64, device="cuda")
    d_c = torch.zeros((batch, r, n), dtype=torch.int64, device="cuda")
    d_out = torch.empty((batch, n), dtype=torch.int64, device="cuda")
    d_status = torch.zeros(batch, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ring.quadform_device(d_out.data_ptr(), d_status.data_ptr(), d_g.data_ptr(), d_c.data_ptr(), batch, r, batch, offdiag, 0, GROUP_BOUND_C,
                             stream=torch.cuda.current_stream().cuda_stream)
    for replay in range(2):
        g, c = base_g.copy(), base_c.copy()
        if replay == 1:
            g, c = g[::-1].copy(), c[::-1].copy()
            c[1, 0, 0] = GROUP_BOUND_C + 1                      # the flags are cleared and set anew inside the graph
        d_g.copy_(_dev(torch, g))
        d_c.copy_(_dev(torch, c))
        graph.replay()
        torch.cuda.synchronize()
        replayed = (_host(d_out).copy(), d_status.cpu().numpy())
        eager = _device(torch, ring, g, c, offdiag, 0, GROUP_BOUND_C)
        assert _same(replayed, eager) and eager[1].tolist() == ([1, 1, 1] if replay == 0 else [1, 0, 1])
        assert _same(eager, _want(g, c, q, offdiag, 0, GROUP_BOUND_C))
    ring.close()


# ---- 8. the verifier's closing equations on the handle ---------------------------------------------------------------------------------
def test_verifier_identities_on_the_handle(pkg):
    """<z, z> = sum g_il c_i c_l and sum_i <phi_i, z> c_i = sum h_il c_i c_l for z = sum_i c_i s_i, every step a call on the handle"""
    n, q, r, width, beta = 64, Q40, 5, 8, 128
    keys = np.arange(1, 13, dtype=np.uint64).reshape(3, 4)
    with pkg.RingMod(q, n, device=0) as ring:
        coeff = ring.coeff_context()
        s = coeff.ring_sample(r * width, pkg.RING_SAMPLE_BOUNDED, beta, keys[0:1]).reshape(r, width, n)
        phi = coeff.ring_sample(r * width, pkg.RING_SAMPLE_UNIFORM, 0, keys[1:2]).reshape(r, width, n)
        c, tries = coeff.ring_challenge(r, 31, 10, 0, keys[2:3])
        assert tries.tolist() == [1] * r
        g, st_g = ring.gram(s, bound_a=beta)
        h, st_h = ring.gram_sym2(phi, s, 0, beta)
        z, st_z = ring.fold(s, c, bound_p=2)
        zz, st_zz = ring.gram(z[None])
        left, st_left = ring.quadform(g, c, 2, bound_c=2)
        assert (st_g, st_h, st_z, st_zz, st_left) == (1, 1, 1, 1, 1)
        assert left.any() and np.array_equal(zz[0], left)
        cross, st_cross = ring.gram(phi, z[None])                                # [r, 1, n]: <phi_i, z>
        right, st_right = ring.quadform(h, c, 1, bound_c=2)
        assert (st_cross, st_right) == (1, 1)
        assert right.any() and np.array_equal(ring.dot(cross[:, 0], c), right)


# ---- 9. the host form past its first staging chunk ---------------------------------------------------------------------------------------
_STAGING_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as entry
pkg = entry.load_package()
data = np.load(sys.argv[2] + "/in.npz")
g, c = data["g"], data["c"]
with pkg.RingMod(int(data["q"]), g.shape[-1], device=0) as ring:
    out = dict(zip(("own", "own_status"), ring.quadform(g, c, 2, 0, 2)))
    out.update(zip(("shared", "shared_status"), ring.quadform(g, c[0], 2, 0, 2)))
np.savez(sys.argv[2] + "/out.npz", **out)
"""


def test_host_form_in_several_staging_chunks_equals_one_chunk(pkg, tmp_path):
    """a fresh child under LAMBDA_SNARK_STAGING_MIB=1 (read once per process): 6 n words a family, five families a chunk, 24 families;
    family 7, in the second chunk, breaks bound_c"""
    assert "LAMBDA_SNARK_STAGING_MIB" not in os.environ, "the reference run takes the default bound"
    q, n, r, batch = 1 << 32, 4096, 2, 24
    assert (1 << 20) // (6 * n * 8) == 5
    rng = np.random.default_rng(24)
    g = rng.integers(0, q, size=(batch, 3, n), dtype=np.uint64)
    c = _bounded(rng, q, (batch, r, n), 2)
    c[7, 1, n - 1] = 3
    with pkg.RingMod(q, n, device=0) as ring:
        own, shared = ring.quadform(g, c, 2, 0, 2), ring.quadform(g, c[0], 2, 0, 2)
    assert own[1].tolist() == [1] * 7 + [0] + [1] * 16 and shared[1].tolist() == [1] * batch and not own[0][7].any() and own[0][23].any()
    for j in (0, 5, 23):                                                             # the first word of a chunk, the last family
        assert np.array_equal(own[0][j], _want(g[j:j + 1], c[j:j + 1], q, 2, 0, 2)[0][0]), j
    np.savez(str(tmp_path / "in.npz"), q=np.uint64(q), g=g, c=c)
    script = tmp_path / "staging_child.py"
    script.write_text(_STAGING_CHILD)
    subprocess.run([sys.executable, str(script), ROOT, str(tmp_path)], check=True, env=dict(os.environ, LAMBDA_SNARK_STAGING_MIB="1"), timeout=300)
    got = np.load(str(tmp_path / "out.npz"))
    assert _same((got["own"], got["own_status"]), own) and _same((got["shared"], got["shared_status"]), shared)
