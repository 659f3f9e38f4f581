"""GPU suite: the masked response z = y + sum c s with its abort under an arbitrary modulus (RingMod.respond / respond_device,
lsr_ring_mod_respond_batch, batch.h "responses under any modulus").  Every output word and every status is compared
exactly with the Python-integer model (tests/ring_mod_respond_model.py: no primes, no groups), or — where the model would take more
than seconds — with RingMod.fold plus an add mod q and a centred maximum in numpy, which the contract names as the definition.
Device outputs are one vector longer than the call needs and come back with that tail untouched; out and status are pre-filled with
sentinels."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import ring_mod_fold_model as fold_model
import ring_mod_model as model
import ring_mod_respond_model as respond_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P5 = model.prime_5_mod_8_below(1 << 32)
Q40 = fold_model.Q40
SENTINEL = 0x5A5A5A5A5A5A5A5A
STATUS_SENTINEL = 7
REJECTED = respond_model.REJECTED


def _dev(torch, x):
    return torch.from_numpy(np.array(x, dtype=np.uint64, order="C").view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _vectors(outputs, terms, stride):
    return (outputs - 1) * stride + terms


def _device_respond(torch, ring, v, p, y, stride, bound_y=0, bound_v=0, bound_p=0, bound_z=0, in_place=False):
    """respond_device on copies of v [vectors, width, n], p [outputs, terms, n] and y [outputs, width, n] (or None): (out, status),
    the guards checked.  in_place: y lies in the output buffer and is passed as out."""
    outputs, terms, n = p.shape
    width = v.shape[1]
    d_v, d_p = _dev(torch, v), _dev(torch, p)
    d_out = torch.full((outputs + 1, width, n), SENTINEL, dtype=torch.int64, device="cuda")
    d_status = torch.full((outputs + 1,), STATUS_SENTINEL, dtype=torch.int32, device="cuda")
    d_y = None
    if y is not None and in_place:
        d_out[:outputs].copy_(_dev(torch, y))
    elif y is not None:
        d_y = _dev(torch, y)
    y_ptr = d_out.data_ptr() if in_place else (d_y.data_ptr() if d_y is not None else 0)
    ring.respond_device(d_out.data_ptr(), d_status.data_ptr(), y_ptr, d_v.data_ptr(), d_p.data_ptr(), outputs, terms, stride, width, bound_y, bound_v,
                        bound_p, bound_z, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out, status = _host(d_out), d_status.cpu().numpy()
    assert bool((out[-1] == np.uint64(SENTINEL)).all()) and status[-1] == STATUS_SENTINEL, "the words behind out or status were written"
    for d, x in ((d_v, v), (d_p, p)) + (((d_y, y),) if d_y is not None else ()):
        assert np.array_equal(_host(d), x), "an operand was written"
    return out[:-1], status[:-1]


def _device_fold(torch, ring, v, p, stride, bound_v=0, bound_p=0):
    outputs, terms, n = p.shape
    d_v, d_p = _dev(torch, v), _dev(torch, p)
    d_out = torch.empty((outputs, v.shape[1], n), dtype=torch.int64, device="cuda")
    d_status = torch.empty((outputs,), dtype=torch.int32, device="cuda")
    ring.fold_device(d_out.data_ptr(), d_status.data_ptr(), d_v.data_ptr(), d_p.data_ptr(), outputs, terms, stride, v.shape[1], bound_v, bound_p,
                     stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return _host(d_out), d_status.cpu().numpy()


def _model(v, p, q, y, stride, bound_y=0, bound_v=0, bound_p=0, bound_z=0):
    out, status = respond_model.respond(v.tolist(), p.tolist(), q, None if y is None else y.tolist(), stride, bound_y, bound_v, bound_p, bound_z)
    return np.array(out, dtype=np.uint64).reshape(p.shape[0], v.shape[1], v.shape[2]), np.array(status, dtype=np.int32)


def _magnitude(x, q):
    """the centred magnitudes of words below q"""
    return np.where(x <= np.uint64(q // 2), x, np.uint64(q) - x)


def _composed(fold, y, q, bound_y=0, bound_z=0):
    """The definition in numpy on top of a fold's (out, status): the add mod q, the checks of y, the centred maximum, the precedence"""
    f, status = fold[0].copy(), fold[1].copy()
    h = q // 2
    by, bz = np.uint64(bound_y or h), np.uint64(bound_z or h)
    z = f
    if y is not None:
        not_below = (y >= np.uint64(q)).any(axis=(1, 2))
        over = ((y < np.uint64(q)) & (_magnitude(y, q) > by)).any(axis=(1, 2))
        status = np.where((status == -1) | not_below, -1, np.where((status == 0) | over, 0, 1)).astype(np.int32)
        z = (f + np.where(y < np.uint64(q), y, np.uint64(0))) % np.uint64(q)
    rejected = (_magnitude(z, q) > bz).any(axis=(1, 2))
    status = np.where((status == 1) & rejected, REJECTED, status).astype(np.int32)
    z[status != 1] = 0
    return z, status


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def _short(rng, q, shape, bound):
    return (rng.integers(-bound, bound + 1, size=shape) % q).astype(np.uint64)


def _mask_for(f, target, q):
    """the y with (f + y) mod q == target"""
    return ((target.astype(np.int64) - f.astype(np.int64)) % q).astype(np.uint64)


def _flavoured(pkg, lib, flavour, q, n):
    lib.lsr_set_arith_mode(0 if flavour == "f64" else 1)
    try:
        ring = pkg.RingMod(q, n, device=0)
    finally:
        lib.lsr_set_arith_mode(0)
    assert ring.prime_context(0).uses_f64 == (flavour == "f64") == ring.prime_context(1).uses_f64
    return ring


# ---- 1. model parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,q", [(2, 2), (4, 3329), (64, P5), (256, 3329), (64, 1 << 32)])
def test_model_parity_host_and_device_at_every_stride(pkg, n, q):
    """outputs 3, terms 3, width 3; shared, disjoint, overlapping and spaced terms; with a mask — bound_z the largest centred word of
    output 0, met exactly — and without; y = None with bound_z = 0 is the fold word for word"""
    import torch
    outputs = terms = width = 3
    h, hp = q // 2, min(q // 2 + 1, q - 1)
    rng = np.random.default_rng(40 + n + q % 1000)
    with pkg.RingMod(q, n, device=0) as ring:
        for stride in (0, 3, 1, 4):
            v = model.planted(rng, q, (_vectors(outputs, terms, stride), width, n), {0: h, 1: hp, 2: h})
            p = model.planted(rng, q, (outputs, terms, n), {0: h, 1: h, 2: hp})
            y = model.planted(rng, q, (outputs, width, n), {0: h, 1: hp})
            fold = ring.fold(v, p, stride)
            assert _same(_device_respond(torch, ring, v, p, None, stride), fold), (n, q, stride, "no mask, device")
            assert _same(ring.respond(v, p, None, stride), fold), (n, q, stride, "no mask, host")
            bound_z = int(_magnitude((fold[0][0] + y[0]) % np.uint64(q), q).max())
            want = _model(v, p, q, y, stride, 0, 0, 0, bound_z)
            assert want[1][0] == 1 and set(want[1].tolist()) <= {1, REJECTED}
            assert _same(_device_respond(torch, ring, v, p, y, stride, 0, 0, 0, bound_z), want), (n, q, stride, "device")
            assert _same(_device_respond(torch, ring, v, p, y, stride, 0, 0, 0, bound_z, in_place=True), want), (n, q, stride, "in place")
            assert _same(ring.respond(v, p, y, stride, 0, 0, 0, bound_z), want), (n, q, stride, "host")
        assert _same(_device_respond(torch, ring, v, p, None, stride), _model(v, p, q, None, stride)), "no mask against the model"
        want = _model(v, p, q, y, stride)
        assert want[1].tolist() == [1, 1, 1] and _same(_device_respond(torch, ring, v, p, y, stride), want), "bound_z = 0 never rejects"
        out, status = ring.respond(v[:terms], p[0], y[0])            # a 2-d p: one output
        assert status == 1 and np.array_equal(out, _model(v[:terms], p[:1], q, y[:1], 0)[0][0])


# ---- 2. the bound on z ---------------------------------------------------------------------------------------------------------------
def test_the_bound_on_z_is_inclusive_and_gates_whole_outputs(pkg):
    """n = 64, q = P5, three outputs.  y = target - f: output 0 has one word of z exactly at bound_z (accepted), output 1 has the last
    word of its last component at -(bound_z + 1) (rejected: all zero, the neighbours intact).  The same output with a word of y over
    bound_y in addition is 0, with a word of y equal to q it is -1."""
    import torch
    q, n, outputs, terms, width, bv, bp, bz = P5, 64, 3, 2, 2, 5, 2, 1000
    by = bz + terms * n * bv * bp                                     # what y = target - f needs
    rng = np.random.default_rng(42)
    v, p = _short(rng, q, (outputs * terms, width, n), bv), _short(rng, q, (outputs, terms, n), bp)
    f, st = fold_model.fold(v.tolist(), p.tolist(), q, terms, bv, bp)
    f = np.array(f, dtype=np.uint64)
    assert st == [1, 1, 1]
    target = _short(rng, q, (outputs, width, n), bz)
    target[0, 0, 7], target[2, 1, 0] = bz, q - bz                     # met exactly, from both sides
    with pkg.RingMod(q, n, device=0) as ring:
        def run(y, want_status):
            want = _model(v, p, q, y, terms, by, bv, bp, bz)
            assert want[1].tolist() == want_status
            for in_place in (False, True):
                got = _device_respond(torch, ring, v, p, y, terms, by, bv, bp, bz, in_place=in_place)
                assert _same(got, want), (want_status, got[1], in_place)
            assert _same(ring.respond(v, p, y, terms, by, bv, bp, bz), want), (want_status, "host")
            for j, s in enumerate(want_status):
                assert bool(got[0][j].any()) == (s == 1)              # a gated output is all zero, its neighbours are not
            return got

        accepted = run(_mask_for(f, target, q), [1, 1, 1])
        assert np.array_equal(accepted[0], target)
        target[1, width - 1, n - 1] = q - bz - 1                      # one over, on the negative side, in the last word there is
        y = _mask_for(f, target, q)
        got = run(y, [1, REJECTED, 1])
        assert np.array_equal(got[0][0], target[0]) and np.array_equal(got[0][2], target[2])
        target[1, width - 1, n - 1] = bz + 1                          # and on the positive side
        run(_mask_for(f, target, q), [1, REJECTED, 1])
        y[1, 0, 5] = by + 1                                           # 0 wins over 2
        run(y, [1, 0, 1])
        y[1, 0, 5] = q - by - 1
        run(y, [1, 0, 1])
        y[1, 1, 9] = q                                                # -1 wins over 0
        run(y, [1, -1, 1])
        y[1, 0, 5] = 0                                                # and over 2
        run(y, [1, -1, 1])


# ---- 3. groups ---------------------------------------------------------------------------------------------------------------------
def test_groups_add_the_mask_once_and_judge_the_finished_sum(pkg):
    """q = 2^40 + 15, n = 64, 9 unbounded terms: groups of 7 + 2.  Output 0: term 0 brings 2^38 into word 0 and term 8 takes it away —
    the sum after the first group is far over bound_z, the finished one within it (accepted).  Output 1: term 8 brings 2^38 into its
    last word (rejected by the finished sum alone).  Output 2: a word >= q in term 8 of v, met when the first group is in out."""
    import torch
    q, n, width, outputs, terms, bz, big = Q40, 64, 2, 3, 9, 5000, 1 << 38
    assert fold_model.groups(q, n, terms) == [7, 2]
    rng = np.random.default_rng(43)
    v, p, y = _short(rng, q, (outputs * terms, width, n), 3), _short(rng, q, (outputs, terms, n), 1), _short(rng, q, (outputs, width, n), 10)
    one = np.zeros(n, dtype=np.uint64)
    one[0] = 1
    p[0, 0], p[0, 8], p[1, 8] = one, one, one
    v[0, 0, 0] = (int(v[0, 0, 0]) + big) % q
    v[8, 0, 0] = (int(v[8, 0, 0]) - big) % q
    with pkg.RingMod(q, n, device=0) as ring:
        first_group = _model(v[:7], p[:1, :7], q, y[:1], 0, 0, 0, 0, bz)
        assert first_group[1].tolist() == [REJECTED]                  # what a norm judged after the first group would say
        want = _model(v, p, q, y, terms, 0, 0, 0, bz)
        assert want[1].tolist() == [1, 1, 1]
        for in_place in (False, True):
            assert _same(_device_respond(torch, ring, v, p, y, terms, 0, 0, 0, bz, in_place=in_place), want), in_place   # y once: the model adds it once
        assert _same(ring.respond(v, p, y, terms, 0, 0, 0, bz), want), "host"
        v[terms + 8, 1, n - 1] = (int(v[terms + 8, 1, n - 1]) + big) % q
        assert _model(v[terms:terms + 7], p[1:2, :7], q, y[1:2], 0, 0, 0, 0, bz)[1].tolist() == [1]
        want = _model(v, p, q, y, terms, 0, 0, 0, bz)
        assert want[1].tolist() == [1, REJECTED, 1] and not want[0][1].any()
        assert _same(_device_respond(torch, ring, v, p, y, terms, 0, 0, 0, bz), want)
        v[2 * terms + 8, 1, n - 1] = q
        want = _model(v, p, q, y, terms, 0, 0, 0, bz)
        assert want[1].tolist() == [1, REJECTED, -1] and not want[0][2].any()
        for in_place in (False, True):
            assert _same(_device_respond(torch, ring, v, p, y, terms, 0, 0, 0, bz, in_place=in_place), want), in_place


# ---- 4. every LT and both flavours -------------------------------------------------------------------------------------------------
def _sweep_width(logn):
    return 2 if logn == 12 else (4096 >> logn) + 3


@functools.lru_cache(maxsize=None)
def _sweep_operands(logn, name):
    """operands of one (n, q): computed once, read-only, shared by the two flavours"""
    n = 1 << logn
    q = model.largest_admissible(n) if name == "top" else P5
    h = q // 2
    width = _sweep_width(logn)
    rng = np.random.default_rng(4000 + 100 * logn + (name == "top"))
    v = model.planted(rng, q, (4, width, n), {0: h, 1: h})          # outputs 2, terms 3, term_stride 1
    p = model.planted(rng, q, (2, 3, n), {0: h, 1: min(h + 1, q - 1)})
    bz = h // 2
    target = _short(rng, q, (2, width, n), bz)
    target[0, 0, 0], target[1, width - 1, n - 1] = bz, q - bz - 1    # output 0 at the bound, output 1 one over it in one word
    for x in (v, p, target):
        x.setflags(write=False)
    return q, v, p, target, bz


@pytest.mark.parametrize("logn", range(1, 13))
@pytest.mark.parametrize("name", ["top", "P5"])
@pytest.mark.parametrize("flavour", ["f64", "u64"])
def test_every_tile_size_flavour_and_modulus_edge(pkg, lib, flavour, name, logn):
    """width = 4096/n + 3 components (a full tile and a ragged one; 2 at n = 4096), 3 terms — under `top` (capacity 1) three groups: a
    first, an accumulating and a last reduce — one output accepted with a word at the bound, one rejected by its last word alone.
    The reference is RingMod.fold with the add and the centred maximum in numpy."""
    import torch
    n = 1 << logn
    q, v, p, target, bz = _sweep_operands(logn, name)
    if name == "top":
        assert fold_model.groups(q, n, 3) == [1, 1, 1]
    with _flavoured(pkg, lib, flavour, q, n) as ring:
        fold = _device_fold(torch, ring, v, p, 1)
        assert fold[1].tolist() == [1, 1]
        y = _mask_for(fold[0], target, q)
        want = _composed(fold, y, q, 0, bz)
        assert want[1].tolist() == [1, REJECTED] and np.array_equal(want[0][0], target[0]) and not want[0][1].any()
        assert _same(_device_respond(torch, ring, v, p, y, 1, 0, 0, 0, bz), want), (flavour, name, n)
        assert _same(_device_respond(torch, ring, v, p, y, 1), _composed(fold, y, q)), (flavour, name, n, "no bound")


# ---- 5. alignment ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _alignment_case(name):
    """n = 64, width 2, 3 outputs of 3 terms, term_stride 1: output 0 accepted, output 1 rejected by one word, output 2 with a word
    of y equal to q.  Under `top` with bound_p = floor(q/2) - 1 every term is its own group; under P5 the call is one group."""
    n, width, outputs, terms = 64, 2, 3, 3
    if name == "top":
        q = model.largest_admissible(n)
        bound_v, bound_p = 0, q // 2 - 1
        assert fold_model.groups(q, n, terms, bound_v, bound_p) == [1, 1, 1]
    else:
        q, bound_v, bound_p = P5, 1 << 20, 2
        assert fold_model.groups(q, n, terms, bound_v, bound_p) == [3]
    rng = np.random.default_rng(45 + (name == "top"))
    vectors = _vectors(outputs, terms, 1)
    v = _short(rng, q, (vectors, width, n), bound_v) if bound_v else model.planted(rng, q, (vectors, width, n), {0: q // 2})
    p = _short(rng, q, (outputs, terms, n), bound_p)
    f = np.array(fold_model.fold(v.tolist(), p.tolist(), q, 1, bound_v, bound_p)[0], dtype=np.uint64)
    bz = q // 4
    target = _short(rng, q, (outputs, width, n), bz)
    target[0, 1, n - 1], target[1, 0, 0] = q - bz, bz + 1
    y = _mask_for(f, target, q)
    y[2, 1, 1] = q
    want = _model(v, p, q, y, 1, 0, bound_v, bound_p, bz)
    assert want[1].tolist() == [1, REJECTED, -1] and want[0][0].any()
    for x in (v, p, y) + want:
        x.setflags(write=False)
    return q, v, p, y, (bound_v, bound_p, bz), want


@pytest.mark.parametrize("name", ["top", "P5"])
@pytest.mark.parametrize("flavour", ["f64", "u64"])
def test_operands_and_outputs_off_the_vector_alignment(pkg, lib, flavour, name):
    """out, y, v and p each start one word into their allocations — 8-byte but not 16-byte aligned — singly and all together, and y
    lies in out itself, aligned and off alignment: the reduce takes 16-byte accesses only where out and y both allow them, the finish
    where out does.  The words around out and behind status stay as they were, and so do the operands."""
    import torch
    n, width, outputs, terms = 64, 2, 3, 3
    q, v, p, y, (bound_v, bound_p, bz), want = _alignment_case(name)
    words = outputs * width * n

    def placed(x, off):
        d = torch.full((x.size + 3,), SENTINEL, dtype=torch.int64, device="cuda")
        assert d.data_ptr() % 16 == 0
        d[off:off + x.size].copy_(_dev(torch, x).reshape(-1))
        return d

    def run(ring, off_out, off_y, off_v, off_p, in_place):
        d_v, d_p = placed(v, off_v), placed(p, off_p)
        d_y = None if in_place else placed(y, off_y)
        d_out = placed(y, off_out) if in_place else torch.full((words + 3,), SENTINEL, dtype=torch.int64, device="cuda")
        d_status = torch.full((outputs + 2,), STATUS_SENTINEL, dtype=torch.int32, device="cuda")
        out_ptr = d_out.data_ptr() + 8 * off_out
        ring.respond_device(out_ptr, d_status.data_ptr(), out_ptr if in_place else d_y.data_ptr() + 8 * off_y, d_v.data_ptr() + 8 * off_v,
                            d_p.data_ptr() + 8 * off_p, outputs, terms, 1, width, 0, bound_v, bound_p, bz, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        out, status = _host(d_out), d_status.cpu().numpy()
        assert (out[:off_out] == SENTINEL).all() and (out[off_out + words:] == SENTINEL).all(), "the words around out were written"
        assert status[outputs:].tolist() == [STATUS_SENTINEL] * 2, "the words behind status were written"
        for d, x, off in ((d_v, v, off_v), (d_p, p, off_p)) + (() if in_place else ((d_y, y, off_y),)):
            got = _host(d)
            assert np.array_equal(got[off:off + x.size], x.reshape(-1)) and (got[:off] == SENTINEL).all() and (got[off + x.size:] == SENTINEL).all(), \
                "an operand was written"
        return out[off_out:off_out + words].reshape(outputs, width, n), status[:outputs]

    with _flavoured(pkg, lib, flavour, q, n) as ring:
        for offsets in ((0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 1, 1, 1)):
            assert _same(run(ring, *offsets, in_place=False), want), (name, flavour, offsets)
        for off_out in (0, 1):
            assert _same(run(ring, off_out, off_out, 1 - off_out, off_out, in_place=True), want), (name, flavour, off_out, "in place")


# ---- 6. chunks ---------------------------------------------------------------------------------------------------------------------
def test_one_output_past_every_chunk_limit(pkg):
    """The fold's shapes (test_ring_mod_fold_gpu.py), each with a mask:
      sums         n = 4096, width 5, terms 2, term_stride 0: 204 outputs fit, outputs = 205 — the rejected output is the one in the
                   second chunk.
      wide output  n = 4096, width 1025: one output alone, its components in chunks of 1024 and 1.  A word of z over bound_z in
                   component 1024 is met when the first 1024 components are in out: the finish zeroes all 1025.  And accepted.
      rows         n = 2, width 1, terms 1: 65537 outputs are sixteen full chunks and one output, which is rejected.
    The reference is RingMod.fold with the add and the centred maximum in numpy."""
    import torch
    rng = np.random.default_rng(46)
    q, n, bz = 1 << 32, 4096, 1 << 20
    with pkg.RingMod(q, n, device=0) as ring:
        outputs, terms, width = 205, 2, 5
        v, p = rng.integers(0, q, size=(terms, width, n), dtype=np.uint64), rng.integers(0, q, size=(outputs, terms, n), dtype=np.uint64)
        fold = _device_fold(torch, ring, v, p, 0)
        target = _short(rng, q, (outputs, width, n), bz)
        target[204, 4, 4095] = q - bz - 1                            # in the second chunk
        y = _mask_for(fold[0], target, q)
        want = _composed(fold, y, q, 0, bz)
        assert want[1].tolist() == [1] * 204 + [REJECTED] and np.array_equal(want[0][:204], target[:204]) and not want[0][204].any()
        assert _same(_device_respond(torch, ring, v, p, y, 0, 0, 0, 0, bz), want)
        assert _same(_device_respond(torch, ring, v, p, y, 0, 0, 0, 0, bz, in_place=True), want)

        outputs, terms, width = 1, 1, 1025
        v, p = _short(rng, q, (1, width, n), 100), rng.integers(0, q, size=(outputs, terms, n), dtype=np.uint64)
        fold = _device_fold(torch, ring, v, p, 1, 100, 0)
        target = _short(rng, q, (outputs, width, n), bz)
        y = _mask_for(fold[0], target, q)
        want = _composed(fold, y, q, 0, bz)
        assert want[1].tolist() == [1] and np.array_equal(want[0], target)
        assert _same(_device_respond(torch, ring, v, p, y, 1, 0, 100, 0, bz), want), "accepted"
        target[0, 1024, 17] = bz + 1
        y = _mask_for(fold[0], target, q)
        want = _composed(fold, y, q, 0, bz)
        assert want[1].tolist() == [REJECTED] and not want[0].any()
        assert _same(_device_respond(torch, ring, v, p, y, 1, 0, 100, 0, bz), want), "rejected in the last component"
        assert _same(_device_respond(torch, ring, v, p, y, 1, 0, 100, 0, bz, in_place=True), want), "rejected in the last component, in place"
    q, n, outputs, bz = 3329, 2, 65537, 1000
    with pkg.RingMod(q, n, device=0) as ring:
        v, p = rng.integers(0, q, size=(outputs, 1, n), dtype=np.uint64), rng.integers(0, q, size=(outputs, 1, n), dtype=np.uint64)
        fold = _device_fold(torch, ring, v, p, 1)
        target = _short(rng, q, (outputs, 1, n), bz)
        target[65536, 0, 1] = bz + 1
        y = _mask_for(fold[0], target, q)
        want = _composed(fold, y, q, 0, bz)
        assert want[1].tolist() == [1] * 65536 + [REJECTED] and np.array_equal(want[0][:65536], target[:65536])
        assert _same(_device_respond(torch, ring, v, p, y, 1, 0, 0, 0, bz), want)


# ---- 7. host staging ---------------------------------------------------------------------------------------------------------------
_STAGED = dict(q=P5, n=64, outputs=40, terms=4, width=64, bound_y=1 << 20, bound_v=1 << 20, bound_p=2)


def _negacyclic_int(a, b):
    """a * b mod X^n + 1 over the integers (int64 arrays of small entries)"""
    n = a.shape[0]
    full = np.convolve(a, b)
    full = np.concatenate([full, np.zeros(2 * n - full.shape[0], dtype=np.int64)])
    return full[:n] - full[n:]


@functools.lru_cache(maxsize=None)
def _staged_operands(stride):
    """n = 64, width 64, 4 terms, 40 outputs: under LAMBDA_SNARK_STAGING_MIB=1 (2048 polynomials per operand) 32, 8 or 29 outputs a
    chunk.  Every operand is short, so z is the integer y + sum c s: bound_z is the median over the outputs of its largest word —
    about half of them are rejected — computed here in numpy.  Output 9 has a challenge over its bound, output 39 one >= q and, with
    term_stride != 0, output 0 a word of v over its bound; output 20 has a word of y over its bound."""
    c = _STAGED
    q, n = c["q"], c["n"]
    rng = np.random.default_rng(47 + stride)
    v = rng.integers(-c["bound_v"], c["bound_v"] + 1, size=(_vectors(c["outputs"], c["terms"], stride), c["width"], n))
    p = rng.integers(-c["bound_p"], c["bound_p"] + 1, size=(c["outputs"], c["terms"], n))
    y = rng.integers(-c["bound_y"], c["bound_y"] + 1, size=(c["outputs"], c["width"], n))
    largest = []
    for j in range(c["outputs"]):
        z = y[j].copy()
        for i in range(c["terms"]):
            for k in range(c["width"]):
                z[k] += _negacyclic_int(v[j * stride + i, k], p[j, i])
        largest.append(int(np.abs(z).max()))
    assert max(largest) < q // 2
    bound_z = sorted(largest)[c["outputs"] // 2]
    v, p, y = (v % q).astype(np.uint64), (p % q).astype(np.uint64), (y % q).astype(np.uint64)
    p[9, 1, 1], p[39, 3, 63] = 3, q
    y[20, 63, 63] = q - c["bound_y"] - 1
    if stride:
        v[0, 63, 63] = c["bound_v"] + 1                           # read by output 0 alone
    for x in (v, p, y):
        x.setflags(write=False)
    return v, p, y, bound_z


def _host_in_place(pkg, ring, v, p, y, stride, bound_y, bound_v, bound_p, bound_z):
    """lsr_ring_mod_respond_batch with y == out: the mask lies in the output buffer"""
    out, status = y.copy(), np.full(p.shape[0], STATUS_SENTINEL, dtype=np.int32)
    v, p = np.ascontiguousarray(v), np.ascontiguousarray(p)
    rc = pkg._abi.load_library().lsr_ring_mod_respond_batch(ring._h, out.ctypes.data, status.ctypes.data, out.ctypes.data, v.ctypes.data, p.ctypes.data,
                                                            p.shape[0], p.shape[1], stride, v.shape[1], bound_y, bound_v, bound_p, bound_z)
    assert rc == 0, pkg._abi.last_error()
    return out, status


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as entry
import test_ring_mod_respond_gpu as t
pkg, c, results = entry.load_package(), t._STAGED, {}
with pkg.RingMod(c["q"], c["n"], device=0) as ring:
    for stride in (0, 4, 1):
        v, p, y, bound_z = t._staged_operands(stride)
        out, status = ring.respond(v, p, y, stride, c["bound_y"], c["bound_v"], c["bound_p"], bound_z)
        results["out%d" % stride], results["status%d" % stride] = out, status
        out, status = t._host_in_place(pkg, ring, v, p, y, stride, c["bound_y"], c["bound_v"], c["bound_p"], bound_z)
        results["in_place_out%d" % stride], results["in_place_status%d" % stride] = out, status
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
            v, p, y, bound_z = _staged_operands(stride)
            want_out, want_status = _device_respond(torch, ring, v, p, y, stride, c["bound_y"], c["bound_v"], c["bound_p"], bound_z)
            assert set(want_status.tolist()) == {1, REJECTED, 0, -1}
            assert want_status[9] == 0 and want_status[20] == 0 and want_status[39] == -1 and (want_status[0] == 0) == (stride != 0)
            for j in np.flatnonzero(want_status == 1):
                assert want_out[j].any()
            assert not want_out[want_status != 1].any()
            assert np.array_equal(got["out%d" % stride], want_out) and np.array_equal(got["status%d" % stride], want_status), stride
            assert np.array_equal(got["in_place_out%d" % stride], want_out) and np.array_equal(got["in_place_status%d" % stride], want_status), stride


# ---- 8. capture --------------------------------------------------------------------------------------------------------------------
def test_graph_capture_as_the_first_call_on_a_fresh_handle(pkg):
    """lsr_ring_mod_create allocated the workspace and there is no prepare: the capture is the handle's first call.  Groups of terms
    inside the graph (7 + 2); two replays on fresh inputs, the second with one rejected output and a word >= q."""
    import torch
    q, n, outputs, terms, width, bz = Q40, 64, 3, 9, 3, 1 << 30
    rng = np.random.default_rng(48)
    vectors = _vectors(outputs, terms, 1)
    d_v = torch.zeros((vectors, width, n), dtype=torch.int64, device="cuda")
    d_p = torch.zeros((outputs, terms, n), dtype=torch.int64, device="cuda")
    d_y = torch.zeros((outputs, width, n), dtype=torch.int64, device="cuda")
    d_out = torch.full((outputs, width, n), SENTINEL, dtype=torch.int64, device="cuda")
    d_status = torch.full((outputs,), STATUS_SENTINEL, dtype=torch.int32, device="cuda")
    with pkg.RingMod(q, n, device=0) as ring, pkg.RingMod(q, n, device=0) as eager:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            ring.respond_device(d_out.data_ptr(), d_status.data_ptr(), d_y.data_ptr(), d_v.data_ptr(), d_p.data_ptr(), outputs, terms, 1, width,
                                bound_z=bz, stream=torch.cuda.current_stream().cuda_stream)
        for replay in range(2):
            v, p = model.planted(rng, q, (vectors, width, n)), model.planted(rng, q, (outputs, terms, n))
            f = np.array(fold_model.fold(v.tolist(), p.tolist(), q, 1)[0], dtype=np.uint64)
            target = _short(rng, q, (outputs, width, n), bz)
            target[0, 0, 0] = bz
            if replay == 1:
                target[1, 2, n - 1] = q - bz - 1                     # rejected
                v[vectors - 1, 2, 0] = q                             # read by the last output alone; the flags are cleared and set anew inside the graph
            y = _mask_for(f, target, q)
            d_v.copy_(_dev(torch, v))
            d_p.copy_(_dev(torch, p))
            d_y.copy_(_dev(torch, y))
            graph.replay()
            torch.cuda.synchronize()
            got = (_host(d_out), d_status.cpu().numpy())
            assert _same(got, _device_respond(torch, eager, v, p, y, 1, 0, 0, 0, bz)) and _same(got, _model(v, p, q, y, 1, 0, 0, 0, bz))
            assert got[1].tolist() == ([1, 1, 1] if replay == 0 else [1, REJECTED, -1])


# ---- 9. a protocol-shaped case -----------------------------------------------------------------------------------------------------
_PROTOCOL_SEED = 49


def test_a_signature_shaped_round_accepts_some_and_rejects_some(pkg):
    """n = 256, q = 8380417, width 5, one term, the secret shared by the 64 instances (term_stride 0): s within 2, the challenges BALL
    of weight 60 from the coefficient context's sampler, the masks within 2^19, bound_z = 2^19 - 120.  |c s| <= 120, so an instance
    with every word of y within 2^19 - 240 is accepted whatever c s is, and one with a word of y beyond 2^19 - 120 is rejected unless
    c s moves that very word back: the seed is one at which y alone, on the CPU, shows instances of the first kind and more than
    eight of the second.  No rate is asserted."""
    import torch
    q, n, width, outputs, kappa, gamma = 8380417, 256, 5, 64, 60, 1 << 19
    bz = gamma - 2 * kappa
    rng = np.random.default_rng(_PROTOCOL_SEED)
    s = _short(rng, q, (1, width, n), 2)
    y_int = rng.integers(-gamma, gamma + 1, size=(outputs, width, n))
    largest = np.abs(y_int).max(axis=(1, 2))
    assert (largest > bz).sum() > 8 and (largest <= bz - 2 * kappa).any()
    y = (y_int % q).astype(np.uint64)
    with pkg.RingMod(q, n, device=0) as ring:
        c = ring.coeff_context().ring_sample(outputs, pkg.RING_SAMPLE_BALL, kappa, pkg.ring_sample_key(_PROTOCOL_SEED)).reshape(outputs, 1, n)
        assert ((c == 1) | (c == q - 1)).sum(axis=(1, 2)).tolist() == [kappa] * outputs and ((c != 0).sum(axis=(1, 2)) == kappa).all()
        fold = _device_fold(torch, ring, s, c, 0, 2, 1)
        assert fold[1].tolist() == [1] * outputs
        want = _composed(fold, y, q, gamma, bz)
        assert set(want[1].tolist()) == {1, REJECTED}
        assert ((want[1] == 1) | (largest > bz - 2 * kappa)).all()    # nothing the mask alone guarantees was rejected
        assert _same(_device_respond(torch, ring, s, c, y, 0, gamma, 2, 1, bz), want)
        assert _same(_device_respond(torch, ring, s, c, y, 0, gamma, 2, 1, bz, in_place=True), want)
        assert _same(ring.respond(s, c, y, 0, gamma, 2, 1, bz), want)
