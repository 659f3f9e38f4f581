"""GPU suite: the Gram, sym2 and quadratic-form kernels — ring_gram_kernel<A, E, SYM, SYM2>, ring_quadform_kernel<A> and
ring_quadform_reduce_kernel<GOLD> behind lsr_ntt_ring_gram_batch, lsr_ntt_ring_gram_sym2_batch and lsr_ntt_ring_quadform_batch (DESIGN.md
§5j, §5m) — held to integer models in six flavours: FP64, u64 at a 60-bit and (forced) at a 44-bit prime, cyclic Goldilocks, and cyclic
contexts over both ordinary primes.

Every output word is compared exactly with the oracle references of ring_gram_model / ring_quadform_model (the CPU oracle's transforms
around pointwise sums on Python integers or the oracle's mul_pointwise) and, at n <= 256, with the schoolbook definitions on Python
integers; at n >= 512 the schoolbook checks one output per form, the last pair of the last family (the quadratic form: the last family
with c per family).  No kernel result is compared with another kernel's.

n = 2 and 16 are part of one 256-lane run of positions, 256 exactly one run, 512 two runs (grid.x = 2), 4096 the largest single-pass
transform, 8192 the smallest two-pass one (the operands go through the other half of the workspace layout).  E = ring_gram_block = 4,
three families (grid.z), width 3:
  cross      (ra, rb) = (1, E + 1), (E + 1, 1), (E, E), (2 E + 1, E + 1), and (E + 1, E + 1) with b the array a (one set of transforms);
  symmetric  r = 1, E, E + 1, 2 E + 1: below one block, one diagonal block, a diagonal and an off-diagonal block with partial blocks;
  sym2       the same r, and r = E + 1 with b the array a: only r > E has a block pair that loads the transposed operands;
  quadform   the same r, c per family and shared, offdiag 1, 2, (q + 1) / 2, q - 1, g random canonical words.  By the slice rule of
             lsr_ring_quadform.hip (restated below) r = 1 is a one-slice launch (the direct store) and every other r a multi-slice one
             (partials and ring_quadform_reduce_kernel, GOLD and not).
At n = 8192 the 2 E + 1 cases are dropped and two families run: still a full block, a partial block and an off-diagonal block pair.

Operands: one pool per (n, q, ring) from ring_tile_model.planted — 0, 1, floor(q/2), floor(q/2) + 1, q - 2, q - 1 at the front of every
polynomial, the Goldilocks carry pool, and goldilocks_lazy_carry(n) as the first column of one vector; a case takes the first ra / rb /
r vectors of every family.  (At n = 2 the planted words fill a polynomial and repeat every three polynomials, the width: every other
polynomial is random there, or all vectors of a family would be equal and a transposed operand no different.)  The pool and the references are computed once, read-only, and shared by the flavours of one modulus and
ring (f64 and u64_q44).  At n >= 512 the last family's a, g and c keep 17 coefficients each (the first 16 and the last): the schoolbook
product costs nonzeros * n there, and their transforms — what the kernels read — are as dense as any.

Each form runs through the host entry and the _device entry.  The device outputs are one polynomial longer than the call owns and
filled with all-ones words, above every modulus: the tail must survive, every owned word must be below q, and the operand buffers on
the device must come back bit-identical.  (test_ring_tile_sweep_gpu's _guarded / _check_guarded fill with a word below the Goldilocks
prime, so this file has its own.)

Then the FP64 re-centring periods (32 columns, 16 for sym2, 32 products and 32 rows in the quadratic form) against the model, and the
flat-spectrum accumulator cases: constant polynomials, whose transform is the constant at every position, so that every
evaluation-domain product is the same residue — floor(q/2) and floor(q/2) + 1 walk an accumulator straight to its bound between
re-centrings — compared with closed forms on Python integers."""
import functools

import numpy as np
import pytest

import ring_quadform_model as quad
from ring_gram_model import oracle_gram, packed_index, pairs, schoolbook_gram
from ring_tile_model import FLAVOURS, GOLDILOCKS, Q60, goldilocks_lazy_carry, omega_for, planted
from test_ring_tile_sweep_gpu import F64_FLAVOURS, _dev, _host, _open, _stream

pytestmark = pytest.mark.gpu

E = 4                                  # ring_gram_block of every flavour (asserted per case)
WIDTH = 3
SIZES = [2, 16, 256, 512, 4096, 8192]
ALL_ONES = -1                          # as int64; 2^64 - 1 as a word: above every modulus
KEPT = 16                              # coefficients a sparse polynomial keeps at its front (and its last one)


def _families(n):
    return 2 if n == 8192 else 3


def _ranks(n):
    return [1, E, E + 1] + ([2 * E + 1] if n < 8192 else [])


def _cases(n):
    """(form, shape): cross (ra, rb); cross_one_set, sym, sym2, sym2_one_set, quadform r"""
    cross = [(1, E + 1), (E + 1, 1), (E, E)] + ([(2 * E + 1, E + 1)] if n < 8192 else [])
    return ([("cross", s) for s in cross] + [("cross_one_set", E + 1)] + [("sym", r) for r in _ranks(n)] + [("sym2", r) for r in _ranks(n)] +
            [("sym2_one_set", E + 1)] + [("quadform", r) for r in _ranks(n)])


def _case_id(case):
    form, shape = case
    return form + "-" + ("%dx%d" % shape if isinstance(shape, tuple) else "r%d" % shape)


SWEEP = [pytest.param(n, case, id="%d-%s" % (n, _case_id(case))) for n in SIZES for case in _cases(n)]


# ---- the slice rule of lsr_ring_quadform.hip, restated ------------------------------------------------------------------------------------
QUAD_THREADS, QUAD_TARGET_GROUPS, QUAD_MIN_SLICE_PAIRS, QUAD_MAX_SLICES = 256, 1024, 4, 64


def _quad_slices(n, families, r):
    """Slices (grid.y) of one launch over the whole triangle of `families` families: as many as bring the launch to
    kQuadTargetGroups workgroups, at least kQuadMinSlicePairs pairs each, at most kQuadMaxSlices.  (The workspace holds every family
    of these shapes with its partials, so nothing else bounds the count.)"""
    npairs = r * (r + 1) // 2
    threads = min(QUAD_THREADS, max(64, n))
    groups = -(-n // threads) * families
    want, most = -(-QUAD_TARGET_GROUPS // groups), -(-npairs // QUAD_MIN_SLICE_PAIRS)
    return max(1, min(want, most, npairs, QUAD_MAX_SLICES))


# ---- operands and references: once per (n, q, ring) -----------------------------------------------------------------------------------------
def _freeze(value):
    for item in value.values() if isinstance(value, dict) else value:
        if isinstance(item, np.ndarray):
            item.setflags(write=False)
        elif isinstance(item, (tuple, list, dict)):
            _freeze(item)
    return value


def _sparse(x):
    x[..., KEPT:-1] = 0


@functools.lru_cache(maxsize=None)
def _operands(n, q, cyclic):
    """a, b [families][R][WIDTH][n], g [families][R (R + 1) / 2][n], c [families][R][n], c_shared [R][n] with R the largest rank at n"""
    families, rmax = _families(n), _ranks(n)[-1]
    npairs = rmax * (rmax + 1) // 2
    rng = np.random.default_rng([n, q % 1000, int(cyclic)])
    def take(*shape):
        x = planted(rng, q, int(np.prod(shape)), n)
        if n < 6:        # the planted words fill the whole polynomial and cycle with a period of 3 polynomials, WIDTH: every vector
            x[1::2] = rng.integers(0, q, size=x[1::2].shape, dtype=np.uint64)      # would be the same one.  Every other one: random
        return x.reshape(shape + (n,))

    ops = {"a": take(families, rmax, WIDTH), "b": take(families, rmax, WIDTH), "g": take(families, npairs), "c": take(families, rmax),
           "c_shared": take(rmax)}
    if q == GOLDILOCKS and n >= 4:         # vector 0 is in every case
        lazy = goldilocks_lazy_carry(n)
        ops["a"][0, 0, 0] = ops["b"][1, 0, 0] = ops["g"][0, 0] = ops["c"][0, 0] = ops["c_shared"][0] = lazy
    if n >= 512:
        for name in ("a", "g", "c"):
            _sparse(ops[name][-1])
    return _freeze(ops)


def _prefix(x, *ranks):
    """a writable, contiguous copy of the first ranks[k] entries along axis 1 + k"""
    return np.array(x[(slice(None),) + tuple(slice(0, r) for r in ranks)], order="C")


def _packed_prefix(x, rmax, r):
    """the packed triangle of the first r vectors out of a triangle packed for rmax: a writable copy [families][r (r + 1) / 2][n]"""
    return np.array(x[:, [packed_index(rmax, i, l) for i, l in pairs(r, r, True)]], order="C")


def _words(nested):
    return np.array(nested, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def _reference(oracle, n, q, cyclic, form):
    """The models' results of one form over the whole pool (a case reads its prefix), computed once and read-only.  "oracle": the
    oracle reference; "school": the schoolbook — everything at n <= 256, {shape: the last pair of the last family} above."""
    ops = _operands(n, q, cyclic)
    omega = omega_for(oracle, next(f for f, v in FLAVOURS.items() if v == (q, cyclic)), n)
    sign = 1 if cyclic else -1
    a, b, rmax, small = ops["a"], ops["b"], _ranks(n)[-1], n <= 256
    ref = lambda fn, *args: fn(oracle, q, n, *args, cyclic, omega)      # noqa: E731
    last = lambda x, r: x[-1:, r - 1:r]                                  # noqa: E731  (vector r - 1 of the last family, as a family of one)
    if form == "cross":
        r = {"oracle": ref(oracle_gram, a, b)}
        r["school"] = _words(schoolbook_gram(a, b, q, sign)) if small else {
            shape: _words(schoolbook_gram(last(a, shape[0]), last(b, shape[1]), q, sign)[0][0][0]) for f, shape in _cases(n) if f == "cross"}
    elif form == "cross_one_set":
        a5 = a[:, :E + 1]
        r = {"oracle": ref(oracle_gram, a5, a5)}
        r["school"] = _words(schoolbook_gram(a5, a5, q, sign) if small else schoolbook_gram(last(a, E + 1), last(a, E + 1), q, sign)[0][0][0])
    elif form == "sym":
        r = {"oracle": ref(oracle_gram, a, None)}
        r["school"] = _words(schoolbook_gram(a, None, q, sign)) if small else {
            k: _words(schoolbook_gram(last(a, k), None, q, sign)[0][0]) for k in _ranks(n)}
    elif form == "sym2":
        r = {"oracle": ref(quad.oracle_sym2, a, b)}
        if small:        # <a_i, b_l> + <a_l, b_i> out of the schoolbook's cross table (the identity: ring_quadform_model's own tests)
            x = _reference(oracle, n, q, cyclic, "cross")["school"].tolist()
            r["school"] = _words([[x[j][i][i] if i == l else quad._add(x[j][i][l], x[j][l][i], q) for i, l in pairs(rmax, rmax, True)]
                                  for j in range(len(x))])
        else:
            r["school"] = {k: _words(quad.schoolbook_sym2(last(a, k), last(b, k), q, sign)[0][0]) for k in _ranks(n)}
    elif form == "sym2_one_set":
        a5 = a[:, :E + 1]
        r = {"oracle": ref(quad.oracle_sym2, a5, a5)}
        r["school"] = _words(quad.schoolbook_sym2(a5, a5, q, sign) if small else quad.schoolbook_sym2(last(a, E + 1), last(a, E + 1), q, sign)[0][0])
    else:                # quadform: {(r, shared): (diag, off)} — a call's words are diag + offdiag * off
        r = {"oracle": {}, "school": {}}
        for k in _ranks(n):
            g = _packed_prefix(ops["g"], rmax, k)
            for shared in (False, True):
                c = ops["c_shared"][:k] if shared else ops["c"][:, :k]
                r["oracle"][k, shared] = ref(quad.oracle_quadform_parts, g, c)
                if small:
                    r["school"][k, shared] = tuple(_words(p) for p in quad.schoolbook_quadform_parts(g, c, q, sign))
                elif not shared:
                    r["school"][k, shared] = tuple(_words(p) for p in quad.schoolbook_quadform_parts(g[-1:], c[-1:], q, sign))
    return _freeze(r)


# ---- the two entry forms ---------------------------------------------------------------------------------------------------------------
def _check_device(torch, d_out, want, q, operands, where):
    """The owned words equal `want` and are below q, the polynomial behind them is untouched, the operands are as they were."""
    torch.cuda.synchronize()
    got = _host(d_out)
    assert bool((got[-1] == np.uint64(2**64 - 1)).all()), (where, "the polynomial behind the output was written")
    assert bool((got[:-1] < np.uint64(q)).all()), (where, "an owned word was not written, or is not canonical")
    assert np.array_equal(got[:-1], want.reshape(got[:-1].shape)), where
    for d_x, x in operands:
        assert np.array_equal(_host(d_x), x), (where, "an operand was written")


def _guard(torch, want, n):
    return torch.full((want.size // n + 1, n), ALL_ONES, dtype=torch.int64, device="cuda")


def _gram_both(torch, ctx, q, form, a, b, want, where):
    """form: cross (b an array, or a itself: one set), sym (b None), sym2 (b an array, or a itself) -> the host form's result"""
    families, ra, width, n = a.shape
    rb = ra if b is None else b.shape[1]
    got = ctx.ring_gram_sym2(a, b) if form == "sym2" else ctx.ring_gram(a, b)
    assert got.shape == want.shape and np.array_equal(got, want), (where, "host")
    d_a = _dev(torch, a)
    d_b = d_a if b is a else None if b is None else _dev(torch, b)
    d_out = _guard(torch, want, n)
    if form == "sym2":
        ctx.ring_gram_sym2_device(d_out.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), families, ra, width, _stream(torch))
    else:
        ctx.ring_gram_device(d_out.data_ptr(), d_a.data_ptr(), None if d_b is None else d_b.data_ptr(), families, ra, rb, width, _stream(torch))
    _check_device(torch, d_out, want, q, [(d_a, a)] + ([] if b is None or b is a else [(d_b, b)]), (where, "device"))
    return got


def _quadform_both(torch, ctx, q, g, c, offdiag, want, where):
    families, _, n = g.shape
    r = c.shape[-2]
    got = ctx.ring_quadform(g, c, offdiag)
    assert got.shape == want.shape and np.array_equal(got, want), (where, "host")
    d_g, d_c, d_out = _dev(torch, g), _dev(torch, c), _guard(torch, want, n)
    ctx.ring_quadform_device(d_out.data_ptr(), d_g.data_ptr(), d_c.data_ptr(), families, r, 1 if c.ndim == 2 else families, offdiag, _stream(torch))
    _check_device(torch, d_out, want, q, [(d_g, g), (d_c, c)], (where, "device"))
    return got


# ---- 1. every flavour, size and block edge ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,case", SWEEP)
@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_every_flavour_size_and_block_edge(pkg, lib, oracle, flavour, n, case):
    import torch
    form, shape = case
    omega = omega_for(oracle, flavour, n)
    q, cyclic, ctx = _open(pkg, lib, flavour, n, omega)
    assert ctx.ring_gram_block == E
    ops, ref = _operands(n, q, cyclic), _reference(oracle, n, q, cyclic, form)
    rmax, small, where = _ranks(n)[-1], n <= 256, (flavour, n, form, shape)
    if form == "quadform":
        r = shape
        families = _families(n)
        assert _quad_slices(n, families, 1) == 1 and (r == 1 or _quad_slices(n, families, r) > 1)
        assert n > 512 or _quad_slices(n, families, 2 * E + 1) > 1                # 45 pairs
        g = _packed_prefix(ops["g"], rmax, r)
        for shared in (False, True):
            c = np.array(ops["c_shared"][:r] if shared else ops["c"][:, :r], order="C")
            for offdiag in (1, 2, (q + 1) // 2, q - 1):
                want = quad.combine_parts(ref["oracle"][r, shared], q, offdiag)
                got = _quadform_both(torch, ctx, q, g, c, offdiag, want, (where, shared, offdiag))
                if (r, shared) in ref["school"]:
                    school = quad.combine_parts(ref["school"][r, shared], q, offdiag)
                    assert np.array_equal(got if small else got[-1:], school), (where, shared, offdiag, "schoolbook")
        ctx.close()
        return
    if form in ("cross", "cross_one_set"):
        ra, rb = shape if form == "cross" else (shape, shape)
        a = _prefix(ops["a"], ra)
        b = a if form == "cross_one_set" else _prefix(ops["b"], rb)
        want = _prefix(ref["oracle"], ra, rb)
        got = _gram_both(torch, ctx, q, "cross", a, b, want, where)
        school = ref["school"][shape] if isinstance(ref["school"], dict) else ref["school"]
        assert np.array_equal(got, school[:, :ra, :rb]) if small else np.array_equal(got[-1, -1, -1], school), (where, "schoolbook")
    else:
        r = shape
        a = _prefix(ops["a"], r)
        b = None if form == "sym" else a if form == "sym2_one_set" else _prefix(ops["b"], r)
        from_pool = form in ("sym", "sym2")          # the pool's triangle is packed for rmax vectors
        want = _packed_prefix(ref["oracle"], rmax, r) if from_pool else np.array(ref["oracle"])
        got = _gram_both(torch, ctx, q, "sym" if form == "sym" else "sym2", a, b, want, where)
        school = ref["school"][r] if isinstance(ref["school"], dict) else ref["school"]
        if small:
            assert np.array_equal(got, _packed_prefix(school, rmax, r) if from_pool else school), (where, "schoolbook")
        else:
            assert np.array_equal(got[-1, -1], school), (where, "schoolbook")
    ctx.close()


# ---- 2. the FP64 re-centring periods against the model ----------------------------------------------------------------------------------
@pytest.mark.parametrize("widths", [(31, 15), (32, 16), (33, 17), (65, 33)], ids=lambda w: "w%d-%d" % w)
@pytest.mark.parametrize("flavour", F64_FLAVOURS)
def test_f64_recentring_periods_of_the_gram_forms(pkg, lib, oracle, flavour, widths):
    """The running sums are re-centred every 32 columns, and every 16 in the sym2 form, which adds two products a column: widths on
    either side of one and of two periods, at r = E + 1 (a diagonal block, an off-diagonal block pair, partial blocks)."""
    import torch
    n, r, families = 256, E + 1, 2
    assert pkg.RING_DOT_F64_RECENTRE_PERIOD == 32
    omega = omega_for(oracle, flavour, n)
    q, cyclic, ctx = _open(pkg, lib, flavour, n, omega)
    assert ctx.ring_gram_block == E                 # (_open asserted the FP64 arithmetic)
    rng = np.random.default_rng([widths[0], int(cyclic)])
    ref = lambda fn, *args: fn(oracle, q, n, *args, cyclic, omega)      # noqa: E731
    for form, width in [("cross", widths[0]), ("sym", widths[0]), ("sym2", widths[1])]:
        a = planted(rng, q, families * r * width, n).reshape(families, r, width, n)
        b = None if form == "sym" else planted(rng, q, families * r * width, n).reshape(families, r, width, n)
        want = ref(quad.oracle_sym2, a, b) if form == "sym2" else ref(oracle_gram, a, b)
        _gram_both(torch, ctx, q, form, a, b, want, (flavour, form, width))
    ctx.close()


@pytest.mark.parametrize("r", [32, 33])
@pytest.mark.parametrize("flavour", F64_FLAVOURS)
def test_f64_recentring_periods_of_the_quadratic_form(pkg, lib, oracle, flavour, r):
    """A row of the triangle has up to r - 1 off-diagonal products and a slice up to r rows: 32 and 33 sit on either side of the period
    of the inner and of the outer sum."""
    import torch
    n, families = 256, 2
    omega = omega_for(oracle, flavour, n)
    q, cyclic, ctx = _open(pkg, lib, flavour, n, omega)             # (asserts the FP64 arithmetic)
    rng = np.random.default_rng([r, int(cyclic)])
    npairs = r * (r + 1) // 2
    g = planted(rng, q, families * npairs, n).reshape(families, npairs, n)
    for c in (planted(rng, q, families * r, n).reshape(families, r, n), planted(rng, q, r, n)):
        parts = quad.oracle_quadform_parts(oracle, q, n, g, c, cyclic, omega)
        for offdiag in (2, q - 1):
            _quadform_both(torch, ctx, q, g, c, offdiag, quad.combine_parts(parts, q, offdiag), (flavour, r, c.ndim, offdiag))
    ctx.close()


# ---- 3. flat spectra: every evaluation-domain product the same residue --------------------------------------------------------------------
def _flat_context(pkg, oracle, name, n):
    """(q, ctx, Gram widths, sym2 widths, quadratic-form ranks)"""
    if name == "f45":
        q = oracle.L.oracle_largest_prime_1mod(2 * n, 45)
        assert 2**44 < q < 2**45
        ctx = pkg.NttContext(q, n, device=0)
        assert ctx.uses_f64
        return q, ctx, (32, 33, 64, 65), (16, 17, 32, 33), (32, 33, 64)
    if name == "q60":
        ctx = pkg.NttContext(Q60, n, device=0)
        assert not ctx.uses_f64
        return Q60, ctx, (41,), (41,), (33,)              # 41 canonical 60-bit summands pass 2^64 unless each sum is reduced
    return GOLDILOCKS, pkg.CyclicNtt(n), (41,), (41,), (33,)


@pytest.mark.parametrize("product", range(4), ids=["half", "half_plus_1", "q_minus_1", "one"])
@pytest.mark.parametrize("name", ["f45", "q60", "gold"])
def test_flat_spectrum_accumulators(pkg, oracle, name, product):
    """a_i[c] = u and b_l[c] = v, constant polynomials: every evaluation-domain product at every position is u v mod q — floor(q/2)
    (centred +q/2), floor(q/2) + 1 (centred -q/2), q - 1, 1 — so a sum walks in one direction for as long as it is not re-centred or
    reduced.  The outputs are constant polynomials with the closed forms of ring_quadform_model, on Python integers."""
    import torch
    n, r, families = 256, E + 1, 2
    q, ctx, widths, widths2, ranks = _flat_context(pkg, oracle, name, n)
    assert ctx.ring_gram_block == E
    u, v = quad.flat_pairs(q)[product]
    assert u * v % q == [q // 2, q // 2 + 1, q - 1, 1][product]
    idx = pairs(r, r, True)
    for width in widths:
        a, b = quad.constant((families, r, width), n, u), quad.constant((families, r, width), n, v)
        _gram_both(torch, ctx, q, "cross", a, b, quad.constant((families, r, r), n, quad.flat_gram(q, width, u, v)), (name, u, v, "cross", width))
        _gram_both(torch, ctx, q, "sym", a, None, quad.constant((families, len(idx)), n, quad.flat_gram(q, width, u, u)), (name, u, "sym", width))
    for width in widths2:
        a, b = quad.constant((families, r, width), n, u), quad.constant((families, r, width), n, v)
        want = np.zeros((families, len(idx), n), dtype=np.uint64)
        want[:, :, 0] = [quad.flat_sym2(q, width, u, v, i == l) for i, l in idx]
        _gram_both(torch, ctx, q, "sym2", a, b, want, (name, u, v, "sym2", width))
    for rank in ranks:
        g = quad.constant((families, rank * (rank + 1) // 2), n, u)
        for c in (quad.constant((families, rank), n, v), quad.constant((rank,), n, v)):
            for offdiag in (1, 2, q - 1):
                want = quad.constant((families,), n, quad.flat_quadform(q, rank, offdiag, u, v))
                _quadform_both(torch, ctx, q, g, c, offdiag, want, (name, u, v, "quadform", rank, c.ndim, offdiag))
    ctx.close()
