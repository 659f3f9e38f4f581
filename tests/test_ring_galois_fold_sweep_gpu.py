"""GPU suite: every arithmetic flavour and every tile log-size LT = 1 .. 12 of the three tile kernels that came after
tests/test_ring_tile_sweep_gpu.py — ring_automorphism_kernel<STAGED> (n <= 4096), ntt_tile_ring_dot_galois<A, LT, BHAT> and
ntt_tile_ring_fold<A, LT, MID = false>.  Each (A, LT) is its own instantiation (1, 2 or 3 rounds, a last round of LT % 4 bits with its
own lane mapping, 4096/n elements per tile and its own ragged-tile clips), so each is launched here, in the six flavours of that sweep:
FP64, u64 at a 60-bit and (forced) at a 44-bit prime, cyclic Goldilocks, and cyclic contexts over both ordinary primes (N = n: the
mask has no sign bit and nothing is negated).

Every word is compared exactly with a CPU reference: the automorphism with the scatter model (ring_galois_model.automorphism_np), the
twisted inner product with galois_dot_ref (the oracle's transforms around a pointwise sum, on the scattered a), the fold with fold_ref
(the same on the gathered operands), and at the first and last element of the full and of the ragged tile with the schoolbook on
Python integers (on the list model's sigma_g(a)), which shares nothing with any transform.  No kernel result is compared with another
kernel's.

Shapes per case: count = batch = width = 4096/n + 3 (one full tile and a ragged one of three elements; 2 at n = 4096), terms = 3, the
fold with two outputs (grid.y = 2).  Every device form writes into an output with one more element behind it, filled with a sentinel
that must survive.

Two combinations do not exist and are asserted: a cyclic context at n = 2 has the single Galois element g = 1, and a shared b needs
batch > 1, which every shape here has."""
import numpy as np
import pytest

import ring_tile_model as model
from ring_fold_model import fold_ref, schoolbook_fold, vectors_needed
from ring_galois_model import (automorphism_batch, automorphism_np, galois_dot_ref, galois_elements, galois_order,
                               test_automorphism_np_equals_the_list_model, test_references_equal_the_schoolbook)  # noqa: F401 (collected here: CPU tests)
from ring_tile_model import FLAVOURS
from test_ring_tile_sweep_gpu import F64_FLAVOURS, _check_guarded, _dev, _edge_vectors, _guarded, _open, _stream


def _distinct_valid(gs, order):
    """The distinct odd elements of gs in [1, N), in order."""
    return [g for i, g in enumerate(gs) if g % 2 == 1 and 1 <= g < order and g not in gs[:i]]


def _scattered(a, g, q, sign):
    """sigma_g(a) by the list model on Python integers (the operand of the schoolbook checks)."""
    return np.array(automorphism_batch(a.tolist(), g, q, sign), dtype=np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("logn", range(1, 13))
@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_every_flavour_and_tile_size(pkg, lib, oracle, flavour, logn):
    import torch
    n = 1 << logn
    omega = model.omega_for(oracle, flavour, n)
    q, cyclic, ctx = _open(pkg, lib, flavour, n, omega)
    sign = 1 if cyclic else -1
    order = galois_order(n, sign)
    assert ctx.galois_conjugation == order - 1
    per_tile = 4096 >> logn
    count = per_tile + 3 if logn < 12 else 2
    edges = _edge_vectors(logn, per_tile, count)
    rng = np.random.default_rng(200 * logn + len(flavour))
    lazy = model.goldilocks_lazy_carry(n) if flavour == "gold" and n >= 4 else None
    where = (flavour, n)
    stream = _stream(torch)

    # 1. the automorphism (STAGED): a full 4096-word run and a ragged one, 0 and q - 1 under both signs
    gs = galois_elements(n, sign) if n <= 16 else _distinct_valid([1, 3, order - 1, order // 2 + 1, order - 5], order)
    if cyclic and n == 2:
        assert gs == [1]                                             # the group of X^2 - 1 is trivial
    else:
        assert len(gs) >= 2 and order - 1 in gs
    x = model.planted(rng, q, count, n)
    d_x = _dev(torch, x)
    for g in gs:
        want = automorphism_np(x, g, q, sign)
        assert np.array_equal(ctx.ring_automorphism(x, g), want), (where, "ring_automorphism", g)
        d_out = _guarded(torch, count, 1, n)
        ctx.ring_automorphism_device(d_out.data_ptr(), d_x.data_ptr(), count, g, stream)
        torch.cuda.synchronize()
        _check_guarded(d_out, want.reshape(count, 1, n), (where, "ring_automorphism_device", g))

    # 2. the twisted inner product: per-output b (BHAT = false) and one shared b (BHAT = true)
    batch, terms = count, 3
    assert batch > 1                                                 # a shared b at batch = 1 is the per-output form: not among these shapes
    dot_gs = [g for g in _distinct_valid([order - 1, order // 2 + 1, 3, order - 5], order) if g != 1][:3]      # g = 1 runs besides these
    if cyclic and n == 2:
        assert not dot_gs
    else:
        assert order - 1 in dot_gs and any(pow(g, -1, order) > order // 2 for g in dot_gs)
    a = model.planted(rng, q, batch * terms, n).reshape(batch, terms, n)
    b = model.planted(rng, q, batch * terms, n).reshape(batch, terms, n)
    if lazy is not None:
        a[1, 0] = b[1, 2] = b[batch - 1, 1] = lazy
    shared = b[batch - 1]
    device_g = dot_gs[0] if dot_gs else 1
    for g in [1] + dot_gs:
        if g == 1:                                                   # sigma_1 is the identity: the plain inner product
            want_each, want_shared = (model.oracle_dot(oracle, q, n, a, rhs, cyclic, omega) for rhs in (b, shared))
        else:
            want_each, want_shared = (galois_dot_ref(oracle, q, n, a, rhs, g, cyclic, omega) for rhs in (b, shared))
        got_each, got_shared = ctx.ring_dot_galois(a, b, g), ctx.ring_dot_galois(a, shared, g)
        assert np.array_equal(got_each, want_each), (where, "ring_dot_galois", g)
        assert np.array_equal(got_shared, want_shared), (where, "ring_dot_galois, shared b", g)
        if edges:
            sa = _scattered(a[edges], g, q, sign)
            assert got_each[edges].tolist() == model.schoolbook_dot(sa, b[edges], q, sign), (where, "ring_dot_galois", g, edges)
            assert got_shared[edges].tolist() == model.schoolbook_dot(sa, shared, q, sign), (where, "ring_dot_galois, shared b", g, edges)
        if g == device_g:                                            # the device form once per case, the b form alternating with LT
            b_rows, rhs, want = (1, shared, want_shared) if logn % 2 else (batch, b, want_each)
            d_a, d_b, d_c = _dev(torch, a), _dev(torch, rhs), _guarded(torch, batch, 1, n)
            ctx.ring_dot_galois_device(d_c.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), batch, terms, b_rows, g, stream)
            torch.cuda.synchronize()
            _check_guarded(d_c, want.reshape(batch, 1, n), (where, "ring_dot_galois_device", g, b_rows))

    # 3. the fold: two outputs, each a full tile of components and a ragged one
    outputs, width = 2, count
    for stride in (1, 0):                                            # overlapping windows (per-output base 1 vector, not `terms`); shared vectors
        v = model.planted(rng, q, vectors_needed(outputs, terms, stride) * width, n).reshape(-1, width, n)
        p = model.planted(rng, q, outputs * terms, n).reshape(outputs, terms, n)
        if lazy is not None:
            v[1, 1] = p[1, 2] = lazy
        want = fold_ref(oracle, q, n, v, p, stride, cyclic, omega)
        got = ctx.ring_fold(v, p, stride)
        assert np.array_equal(got, want), (where, "ring_fold", stride)
        if edges:
            assert got[:, edges].tolist() == schoolbook_fold(v[:, edges], p, stride, q, sign), (where, "ring_fold", stride, edges)
        if stride == 1:
            d_v, d_p, d_out = _dev(torch, v), _dev(torch, p), _guarded(torch, outputs, width, n)
            ctx.ring_fold_device(d_out.data_ptr(), d_v.data_ptr(), d_p.data_ptr(), outputs, terms, stride, width, stream)
            torch.cuda.synchronize()
            _check_guarded(d_out, want, (where, "ring_fold_device", stride))
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("logn", [5, 10, 11])
@pytest.mark.parametrize("flavour", F64_FLAVOURS)
def test_f64_accumulator_through_the_permuted_load(pkg, lib, oracle, flavour, logn):
    """Last rounds of 1, 2 and 3 bits.  33 identical terms under the conjugation g = N - 1: every accumulator receives the same product
    33 times, every one of one sign per residue, across the re-centring after term 31; c = 33 (sigma_g(a0) b0), the single product by
    the oracle on the list model's sigma_g(a0)."""
    n = 1 << logn
    omega = model.omega_for(oracle, flavour, n)
    q, cyclic, ctx = _open(pkg, lib, flavour, n, omega)
    assert pkg.RING_DOT_F64_RECENTRE_PERIOD == 32
    sign = 1 if cyclic else -1
    g, terms, batch = galois_order(n, sign) - 1, 33, 2
    rng = np.random.default_rng(3 * logn + len(flavour))
    a0, b0 = model.planted(rng, q, 1, n), model.planted(rng, q, 1, n)
    one = model.oracle_product(oracle, q, n, _scattered(a0, g, q, sign), b0, cyclic, omega)[0]
    want = np.array([int(v) * terms % q for v in one], dtype=np.uint64)
    a = np.ascontiguousarray(np.broadcast_to(a0[0], (batch, terms, n)))
    for b_shape in [(terms, n), (batch, terms, n)]:
        got = ctx.ring_dot_galois(a, np.ascontiguousarray(np.broadcast_to(b0[0], b_shape)), g)
        assert got.shape == (batch, n)
        for j in range(batch):
            assert np.array_equal(got[j], want), (flavour, n, b_shape, j)
    ctx.close()
