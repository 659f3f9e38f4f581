"""GPU suite: Gram matrices of bounded ring vectors under an arbitrary modulus (RingMod.gram* : lsr_ring_mod_gram_*, batch.h "Gram
matrices under any modulus") against the Python-integer model (tests/ring_mod_gram_model.py) and against the handle's
own fused inner product.  Every comparison is exact, word for word.  Shapes are the smallest at which each mechanism can fail:
ra = 5 against rb = 3 (one full block of 4 and a ragged one, and a diagonal block), width 3, batch 3; widths just above a capacity
(column groups reduced with accumulate); bounds met exactly and missed by one; one family past a chunk of whole families and one
family past the workspace at n = 4096; n = 8192 for the two-pass transforms."""
import functools
import os
import re

import numpy as np
import pytest

import ring_mod_gram_model as model
import ring_mod_model as mod

pytestmark = pytest.mark.gpu

P5 = mod.prime_5_mod_8_below(1 << 32)
Q40 = model.Q40                            # odd, 41 bits: max_terms = 7 at n = 64
RA, RB, WIDTH, BATCH = 5, 3, 3, 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(torch, x):
    return torch.from_numpy(np.array(x, dtype=np.uint64, order="C").view(np.int64)).cuda()          # (a copy: the references are read-only)


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _random(rng, q, shape, bound=0):
    if not bound:
        return rng.integers(0, q, size=shape, dtype=np.uint64)
    v = rng.integers(-bound, bound + 1, size=shape, dtype=np.int64)
    return np.where(v < 0, v + q, v).astype(np.uint64)


def _with_extremes(x, q):
    """the centred extremes floor(q/2) and floor(q/2) + 1 in whole polynomials"""
    x[0, 0, 0, :] = q // 2
    x[1, 1, 0, :] = min(q // 2 + 1, q - 1)
    return x


def _want(pair, shape):
    """the model's (lists, statuses) as arrays"""
    g, status = pair
    return np.array(g, dtype=np.uint64).reshape(shape), np.array(status, dtype=np.int32)


def _device(torch, ring, a, b, bound_a=0, bound_b=0, sym2=False):
    """gram_device / gram_sym2_device on numpy operands ([batch][r][width][n]; b None: symmetric; b is a: one buffer) -> (g, status);
    g and status are pre-filled, so what comes back was written"""
    batch, ra, width, n = a.shape
    d_a = _dev(torch, a)
    d_b = None if b is None else (d_a if b is a else _dev(torch, b))
    rb = ra if b is None else b.shape[1]
    shape = (batch, ra * (ra + 1) // 2, n) if b is None or sym2 else (batch, ra, rb, n)
    d_g = torch.full(shape, -1, dtype=torch.int64, device="cuda")
    d_status = torch.full((batch,), 7, dtype=torch.int32, device="cuda")
    if sym2:
        ring.gram_sym2_device(d_g.data_ptr(), d_status.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), batch, ra, width, bound_a, bound_b, stream=_stream(torch))
    else:
        ring.gram_device(d_g.data_ptr(), d_status.data_ptr(), d_a.data_ptr(), None if d_b is None else d_b.data_ptr(), batch, ra, rb, width, bound_a, bound_b,
                         stream=_stream(torch))
    torch.cuda.synchronize()
    return _host(d_g), d_status.cpu().numpy()


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@functools.lru_cache(maxsize=None)
def _parity_reference(n, q):
    rng = np.random.default_rng(3400 * n + q % 997)
    a, b = _with_extremes(_random(rng, q, (BATCH, RA, WIDTH, n)), q), _with_extremes(_random(rng, q, (BATCH, RB, WIDTH, n)), q)
    b5 = _with_extremes(_random(rng, q, (BATCH, RA, WIDTH, n)), q)
    pairs = RA * (RA + 1) // 2
    want = {"cross": _want(model.gram(a, b, q), (BATCH, RA, RB, n)), "sym": _want(model.gram(a, None, q), (BATCH, pairs, n)),
            "self": _want(model.gram(a, a, q), (BATCH, RA, RA, n)), "sym2": _want(model.gram_sym2(a, b5, q), (BATCH, pairs, n))}
    for arr in (a, b, b5) + tuple(w[0] for w in want.values()):
        arr.setflags(write=False)
    return a, b, b5, want


# ---- 1. model parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,q", [(2, 2), (4, 3329), (64, P5), (256, 3329), (64, 1 << 32)])
def test_three_forms_equal_the_model_host_and_device(pkg, n, q):
    import torch
    a, b, b5, want = _parity_reference(n, q)
    ones = np.ones(BATCH, dtype=np.int32)
    with pkg.RingMod(q, n, device=0) as ring:
        for got in (ring.gram(a, b), _device(torch, ring, a, b)):
            assert _same(got, want["cross"]) and np.array_equal(got[1], ones)
        for got in (ring.gram(a), _device(torch, ring, a, None)):
            assert _same(got, want["sym"]) and np.array_equal(got[1], ones)
        for got in (ring.gram_sym2(a, b5), _device(torch, ring, a, b5, sym2=True)):
            assert _same(got, want["sym2"]) and np.array_equal(got[1], ones)
        for got in (ring.gram(a, a), _device(torch, ring, a, a)):                       # b == a: one set of transforms
            assert _same(got, want["self"])
            for i in range(RA):
                for l in range(i, RA):
                    assert np.array_equal(got[0][:, i, l], want["sym"][0][:, model.index(RA, i, l)]), (i, l)
        g1, s1 = ring.gram(a[0], b[0])                                                   # 3-d operands: a batch of one
        assert np.array_equal(g1, want["cross"][0][0]) and s1 == 1


# ---- 2. the handle's own inner product, pair by pair --------------------------------------------------------------------------------
def test_entries_equal_the_fused_inner_product_pair_by_pair(pkg):
    import torch
    n, q = 64, P5
    a, b, b5, _ = _parity_reference(n, q)
    with pkg.RingMod(q, n, device=0) as ring:
        cross, _ = _device(torch, ring, a, b)
        sym2, _ = _device(torch, ring, a, b5, sym2=True)
        d_c = torch.empty((2, n), dtype=torch.int64, device="cuda")

        def dot(x, y):
            d_x, d_y = _dev(torch, x), _dev(torch, y)
            ring.dot_device(d_c.data_ptr(), d_x.data_ptr(), d_y.data_ptr(), 1, WIDTH, 1, stream=_stream(torch))
            torch.cuda.synchronize()
            return _host(d_c)[0].copy()

        for j in range(BATCH):
            for i in range(RA):
                for l in range(RB):
                    assert np.array_equal(cross[j, i, l], dot(a[j, i], b[j, l])), (j, i, l)
        j = 1
        for i in range(RA):
            for l in range(i, RA):
                both = dot(a[j, i], b5[j, l]) if i == l else (dot(a[j, i], b5[j, l]) + dot(a[j, l], b5[j, i])) % np.uint64(q)
                assert np.array_equal(sym2[j, model.index(RA, i, l)], both), (i, l)


# ---- 3. capacity groups -------------------------------------------------------------------------------------------------------------
def test_column_groups_follow_the_capacity_of_the_stated_bounds(pkg):
    """q = 2^40 + 15, n = 64: no bounds — 7 columns a group (sym2: 3); b within 2^37 — 31; both within 128 — any width is one group"""
    import torch
    n, q, h = 64, Q40, Q40 // 2
    rng = np.random.default_rng(17)
    with pkg.RingMod(q, n, device=0) as ring:
        assert ring.max_terms == 7 == pkg.ring_mod_capacity_product(q, n, h, h)
        a, b = _random(rng, q, (2, RA, 17, n)), _random(rng, q, (2, RB, 17, n))            # 7 + 7 + 3
        assert _same(_device(torch, ring, a, b), _want(model.gram(a, b, q), (2, RA, RB, n)))
        assert _same(ring.gram(a), _want(model.gram(a, None, q), (2, RA * (RA + 1) // 2, n)))
        b5 = _random(rng, q, (2, RA, 17, n))                                               # sym2: 3 + 3 + 3 + 3 + 3 + 2
        assert pkg.ring_mod_capacity_product(q, n, h, h) // 2 == 3
        assert _same(_device(torch, ring, a, b5, sym2=True), _want(model.gram_sym2(a, b5, q), (2, RA * (RA + 1) // 2, n)))
        assert pkg.ring_mod_capacity_product(q, n, h, 1 << 37) == 31                        # 31 + 2
        a, b = _random(rng, q, (2, RA, 33, n)), _random(rng, q, (2, RB, 33, n), bound=1 << 37)
        b[0, 0, 32, 0], b[1, 2, 0, 5] = 1 << 37, q - (1 << 37)
        got = _device(torch, ring, a, b, 0, 1 << 37)
        assert _same(got, _want(model.gram(a, b, q, 0, 1 << 37), (2, RA, RB, n))) and got[1].tolist() == [1, 1]
        assert pkg.ring_mod_capacity_product(q, n, 128, 128) == 2**64 - 1                   # one group
        a, b = _random(rng, q, (2, RA, 33, n), bound=128), _random(rng, q, (2, RB, 33, n), bound=128)
        got = _device(torch, ring, a, b, 128, 128)
        assert _same(got, _want(model.gram(a, b, q, 128, 128), (2, RA, RB, n))) and got[1].tolist() == [1, 1]
        assert _same(ring.gram(a, b, 128, 128), got)


# ---- 4. bound enforcement -----------------------------------------------------------------------------------------------------------
def _enforcement_operands(rng, q, n, width, bound_a, bound_b, in_b, negative):
    """family 0 meets the bounds exactly, family 1 misses one by one in a single word of the LAST column, family 2 holds a word equal
    to q, one above q and an over-bound word"""
    a, b = _random(rng, q, (3, RA, width, n), bound=bound_a), _random(rng, q, (3, RB, width, n), bound=bound_b)
    edge_a, edge_b = bound_a or q // 2, bound_b or q // 2
    a[0, 1, 0, 3], a[0, 4, width - 1, n - 1] = edge_a, q - edge_a
    b[0, 0, width - 1, 0], b[0, 2, 0, 7] = edge_b, q - edge_b
    over = (edge_b if in_b else edge_a) + 1
    (b if in_b else a)[1, 2, width - 1, n // 2] = q - over if negative else over
    a[2, 0, width - 1, 1], b[2, 1, 0, 0], b[2, 2, width - 1, 2] = q, q + 5, edge_b + 1
    return a, b


@pytest.mark.parametrize("in_b,negative", [(False, False), (True, True)])
def test_bounds_are_verified_per_family(pkg, in_b, negative):
    """bound 128 on both operands; +129 in a, or -129 in b only"""
    import torch
    n, q, bound = 64, P5, 128
    a, b = _enforcement_operands(np.random.default_rng(128 + in_b), q, n, WIDTH, bound, bound, in_b, negative)
    want = _want(model.gram(a, b, q, bound, bound), (3, RA, RB, n))
    assert want[1].tolist() == [1, 0, -1] and want[0][0].any() and not want[0][1:].any()
    with pkg.RingMod(q, n, device=0) as ring:
        assert _same(_device(torch, ring, a, b, bound, bound), want)
        assert _same(ring.gram(a, b, bound, bound), want)
        sym = _device(torch, ring, a, None, bound, 1)                                     # the symmetric form does not read bound_b
        assert _same(sym, _want(model.gram(a, None, q, bound), (3, RA * (RA + 1) // 2, n))) and sym[1].tolist() == [1, 1 if in_b else 0, -1]
        b5 = np.concatenate([b, b[:, :2]], axis=1)
        got = _device(torch, ring, a, b5, bound, bound, sym2=True)
        assert _same(got, _want(model.gram_sym2(a, b5, q, bound, bound), (3, RA * (RA + 1) // 2, n))) and got[1].tolist() == [1, 0, -1]
        # b == a: the same words against both bounds
        first = a[:1]
        assert _device(torch, ring, first, first, bound, bound)[1].tolist() == [1]
        got = _device(torch, ring, first, first, bound, bound - 1)
        assert got[1].tolist() == [0] and not got[0].any()
        # no bounds: only -1 can occur
        none = _device(torch, ring, a, b)
        assert _same(none, _want(model.gram(a, b, q), (3, RA, RB, n))) and none[1].tolist() == [1, 1, -1]


@pytest.mark.parametrize("negative", [False, True])
def test_flags_are_complete_before_the_first_reduce_of_a_family_in_column_groups(pkg, negative):
    """q = 2^40 + 15, no bound on a, b within 2^38: 14 columns a group, width 17, and every offending word sits in the LAST group —
    the outputs of the first group are zeros all the same.  (No bound on either operand has capacity 7 but cannot miss a bound; a
    bound of 128 on b alone makes every width one group.)"""
    import torch
    n, q, width, bound_b = 64, Q40, 17, 1 << 38
    capacity = pkg.ring_mod_capacity_product(q, n, q // 2, bound_b)
    assert capacity == model.capacity_product(q, n, q // 2, bound_b) and width - capacity in range(1, capacity)
    a, b = _enforcement_operands(np.random.default_rng(38 + negative), q, n, width, 0, bound_b, True, negative)
    want = _want(model.gram(a, b, q, 0, bound_b), (3, RA, RB, n))
    assert want[1].tolist() == [1, 0, -1]
    with pkg.RingMod(q, n, device=0) as ring:
        assert _same(_device(torch, ring, a, b, 0, bound_b), want)
        assert _same(ring.gram(a, b, 0, bound_b), want)


# ---- 4b. operands and outputs off the vector alignment ---------------------------------------------------------------------------------
def test_operands_and_outputs_off_the_vector_alignment(pkg):
    """a, b and g start one word into their allocations: 8-byte but not 16-byte aligned, where the host takes the one-word-per-lane
    variants of the lift and of the reduce.  Width 3 within 128 is one group (the check rides in the lift); width 9 without bounds
    is above the capacity of 7 (a check-only pass, lifts without the check, a plain and an accumulating reduce); a word at
    bound + 1 zeroes its family.  The words around g and behind status stay as they were."""
    import torch
    n, q, ra, rb, batch, bound = 64, Q40, 3, 2, 2, 128
    sentinel, status_sentinel = 0x5A5A5A5A5A5A5A5A, 7
    assert mod.capacity(q, n) == 7
    rng = np.random.default_rng(816)

    def off_alignment(x):
        d = torch.full((x.size + 2,), sentinel, dtype=torch.int64, device="cuda")
        d[1:1 + x.size].copy_(_dev(torch, x).reshape(-1))
        assert (d.data_ptr() + 8) % 16 == 8
        return d

    def run(ring, a, b, bound_a, bound_b):
        d_a, d_b = off_alignment(a), off_alignment(b)
        words = batch * ra * rb * n
        d_g = torch.full((words + 3,), sentinel, dtype=torch.int64, device="cuda")
        d_status = torch.full((batch + 2,), status_sentinel, dtype=torch.int32, device="cuda")
        assert (d_g.data_ptr() + 8) % 16 == 8
        ring.gram_device(d_g.data_ptr() + 8, d_status.data_ptr(), d_a.data_ptr() + 8, d_b.data_ptr() + 8, batch, ra, rb, a.shape[2], bound_a, bound_b,
                         stream=_stream(torch))
        torch.cuda.synchronize()
        g, status = _host(d_g), d_status.cpu().numpy()
        assert g[0] == sentinel and (g[1 + words:] == sentinel).all(), "the words around g were written"
        assert status[batch:].tolist() == [status_sentinel] * 2, "the words behind status were written"
        for d, x in ((d_a, a), (d_b, b)):
            assert np.array_equal(_host(d)[1:-1], x.reshape(-1)) and _host(d)[0] == sentinel == _host(d)[-1]
        return g[1:1 + words].reshape(batch, ra, rb, n), status[:batch]

    with pkg.RingMod(q, n, device=0) as ring:
        a, b = _random(rng, q, (batch, ra, 3, n), bound=bound), _random(rng, q, (batch, rb, 3, n), bound=bound)
        a[0, 0, 0, 0], a[1, 2, 2, n - 1], b[0, 1, 2, 5], b[1, 0, 0, 0] = bound, q - bound, q - bound, bound       # the bounds met exactly
        assert pkg.ring_mod_capacity_product(q, n, bound, bound) >= 3
        want = _want(model.gram(a, b, q, bound, bound), (batch, ra, rb, n))
        assert want[1].tolist() == [1, 1] and _same(run(ring, a, b, bound, bound), want)

        width = 9                                                                # 7 + 2
        assert ring.max_terms == 7 == pkg.ring_mod_capacity_product(q, n, q // 2, q // 2) < width
        wide_a, wide_b = _with_extremes(_random(rng, q, (batch, ra, width, n)), q), _with_extremes(_random(rng, q, (batch, rb, width, n)), q)
        want = _want(model.gram(wide_a, wide_b, q), (batch, ra, rb, n))
        assert want[1].tolist() == [1, 1] and _same(run(ring, wide_a, wide_b, 0, 0), want)

        b[1, 1, 2, n - 1] = bound + 1
        want = _want(model.gram(a, b, q, bound, bound), (batch, ra, rb, n))
        got = run(ring, a, b, bound, bound)
        assert want[1].tolist() == [1, 0] and want[0][0].any() and _same(got, want) and not got[0][1].any()


# ---- 5. workspace edges -------------------------------------------------------------------------------------------------------------
def _workspace_words():
    """per prime, as batch.h states it"""
    text = open(os.path.join(ROOT, "include", "lambda_snark", "batch.h")).read()
    m = re.search(r"per prime max\(2\^(\d+), LAMBDA_SNARK_NTT_CHUNK_MIB 2\^20 / (\d+)\)", text)
    assert m, "batch.h states the size of the Gram workspace"
    chunk_mib = int(os.environ.get("LAMBDA_SNARK_NTT_CHUNK_MIB", "0") or 0)
    return max(1 << int(m.group(1)), (chunk_mib if chunk_mib > 0 else 256) * (1 << 20) // int(m.group(2)))


def _pairs_by_dot(torch, ring, d_a, j, r, width, n):
    """the packed symmetric entries of family j of d_a [batch][r][width][n] through the fused inner product"""
    d_c = torch.empty((r * (r + 1) // 2, n), dtype=torch.int64, device="cuda")
    for i in range(r):
        for l in range(i, r):
            ring.dot_device(d_c[model.index(r, i, l)].data_ptr(), d_a[j, i].data_ptr(), d_a[j, l].data_ptr(), 1, width, 1, stream=_stream(torch))
    return d_c


def test_one_family_past_a_chunk_of_whole_families(pkg):
    import torch
    n, q, r = 4096, 1 << 32, 2
    polys = _workspace_words() // n
    width = polys // 8                                           # (2 width + 3) polynomials a family: three families a chunk
    chunk = polys // (r * width + 3)
    assert chunk == 3
    batch = chunk + 1
    torch.manual_seed(5)
    d_a = torch.randint(0, q, (batch, r, width, n), dtype=torch.int64, device="cuda")
    d_g = torch.full((batch, 3, n), -1, dtype=torch.int64, device="cuda")
    d_status = torch.zeros(batch, dtype=torch.int32, device="cuda")
    with pkg.RingMod(q, n, device=0) as ring:
        ring.gram_device(d_g.data_ptr(), d_status.data_ptr(), d_a.data_ptr(), None, batch, r, r, width, stream=_stream(torch))
        for j in (0, chunk - 1, chunk):
            assert torch.equal(d_g[j], _pairs_by_dot(torch, ring, d_a, j, r, width, n)), j
        assert d_status.tolist() == [1] * batch


def test_one_family_past_the_workspace_takes_column_groups(pkg):
    """2 width polynomials of operands alone fill the workspace: groups of (polys - 3) / 2 columns, then the rest; the second family
    breaks its bound in the last group"""
    import torch
    n, q, r, batch, bound = 4096, 1 << 32, 2, 2, 1 << 20
    polys = _workspace_words() // n
    width = polys // 2
    assert r * width + 3 > polys >= r + 3 and pkg.ring_mod_capacity_product(q, n, bound, bound) >= width
    torch.manual_seed(6)
    d_a = torch.randint(0, bound + 1, (batch, r, width, n), dtype=torch.int64, device="cuda")
    d_a[1, 1, width - 1, n - 1] = bound + 1
    d_g = torch.full((batch, 3, n), -1, dtype=torch.int64, device="cuda")
    d_status = torch.zeros(batch, dtype=torch.int32, device="cuda")
    with pkg.RingMod(q, n, device=0) as ring:
        ring.gram_device(d_g.data_ptr(), d_status.data_ptr(), d_a.data_ptr(), None, batch, r, r, width, bound, stream=_stream(torch))
        assert torch.equal(d_g[0], _pairs_by_dot(torch, ring, d_a, 0, r, width, n))
        assert d_status.tolist() == [1, 0] and not bool(d_g[1].any())


# ---- 6. n above 4096 ----------------------------------------------------------------------------------------------------------------
def test_n_8192_on_sampled_coefficients(pkg):
    import torch
    n, q, r, width, batch = 8192, 1 << 32, 2, 2, 2
    rng = np.random.default_rng(8192)
    a, b = _random(rng, q, (batch, r, width, n)), _random(rng, q, (batch, r, width, n))
    positions = sorted({0, 1, n // 2, n - 2, n - 1} | set(rng.integers(0, n, size=5).tolist()))
    with pkg.RingMod(q, n, device=0) as ring:
        cross, status = _device(torch, ring, a, b)
        sym, _ = ring.gram(a)
        sym2, _ = _device(torch, ring, a, b, sym2=True)
        assert status.tolist() == [1, 1]
        for j in range(batch):
            for i in range(r):
                for l in range(r):
                    coeffs = [mod.dot_coefficient(a[j, i], b[j, l], q, k) for k in positions]
                    assert [int(cross[j, i, l, k]) for k in positions] == coeffs, (j, i, l)
                    if i < l:
                        other = [mod.dot_coefficient(a[j, l], b[j, i], q, k) for k in positions]
                        assert [int(sym2[j, model.index(r, i, l), k]) for k in positions] == [(u + v) % q for u, v in zip(coeffs, other)], (j, i, l)
                    if i <= l:
                        assert [int(sym[j, model.index(r, i, l), k]) for k in positions] == [mod.dot_coefficient(a[j, i], a[j, l], q, k) for k in positions]


# ---- 7. capture ---------------------------------------------------------------------------------------------------------------------
def test_graph_capture_after_prepare(pkg):
    """no eager call first: gram_prepare allocated the workspace.  Column groups inside the graph; two replays on fresh inputs."""
    import torch
    n, q, width, batch = 64, Q40, 9, 2                           # 7 + 2
    rng = np.random.default_rng(77)
    ring = pkg.RingMod(q, n, device=0)
    ring.gram_prepare()
    ring.gram_prepare()                                          # idempotent
    d_a = torch.zeros((batch, RA, width, n), dtype=torch.int64, device="cuda")
    d_b = torch.zeros((batch, RB, width, n), dtype=torch.int64, device="cuda")
    d_g = torch.empty((batch, RA, RB, n), dtype=torch.int64, device="cuda")
    d_status = torch.zeros(batch, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ring.gram_device(d_g.data_ptr(), d_status.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), batch, RA, RB, width, stream=torch.cuda.current_stream().cuda_stream)
    for replay in range(2):
        a, b = _random(rng, q, (batch, RA, width, n)), _random(rng, q, (batch, RB, width, n))
        if replay == 1:
            b[1, 0, width - 1, 0] = q                           # the flags are cleared and set anew inside the graph
        d_a.copy_(_dev(torch, a))
        d_b.copy_(_dev(torch, b))
        graph.replay()
        torch.cuda.synchronize()
        assert _same((_host(d_g), d_status.cpu().numpy()), _want(model.gram(a, b, q), (batch, RA, RB, n)))
        assert d_status.tolist() == ([1, 1] if replay == 0 else [1, -1])
    ring.close()


def test_capture_without_the_workspace_is_refused_and_leaves_the_handle_usable(pkg):
    import torch
    n, q = 64, P5
    a, b, _, want = _parity_reference(n, q)
    d_a, d_b = _dev(torch, a), _dev(torch, b)
    d_g = torch.zeros((BATCH, RA, RB, n), dtype=torch.int64, device="cuda")
    d_status = torch.zeros(BATCH, dtype=torch.int32, device="cuda")
    with pkg.RingMod(q, n, device=0) as ring:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            d_g.add_(0)                    # (keeps the captured graph non-empty)
            rc = ring._lib.lsr_ring_mod_gram_batch_device(ring.handle, d_g.data_ptr(), d_status.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), BATCH, RA, RB, WIDTH,
                                                          0, 0, torch.cuda.current_stream().cuda_stream)
        assert rc == -1
        msg = pkg._abi.last_error()
        assert msg.startswith("lsr_ring_mod_gram_batch_device:") and "workspace" in msg and "eager" in msg
        graph.replay()                     # the capture stayed usable
        torch.cuda.synchronize()
        assert not bool(d_g.any())         # and holds no launch of the refused call
        assert _same(_device(torch, ring, a, b), want["cross"])


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_in_the_documented_order_on_a_real_handle(pkg):
    """each with a later fault behind it that must not be the one reported"""
    import torch
    n, q = 64, P5
    h = q // 2
    d = [torch.zeros((2, 2, 2, n), dtype=torch.int64, device="cuda") for _ in range(3)]
    d_status = torch.zeros(2, dtype=torch.int32, device="cuda")
    g, a, b, st = d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d_status.data_ptr()
    with pkg.RingMod(q, n, device=0) as ring:
        lib = ring._lib

        def cross(word, *args):
            assert lib.lsr_ring_mod_gram_batch_device(ring.handle, *args, None) == -1
            assert word in pkg._abi.last_error(), pkg._abi.last_error()

        cross("NULL", g, None, a, b, 1, 0, 2, 2, 0, 0)                       # (1) before (2)
        cross("at least 1", g, st, a, b, 1, 0, 65, 2, 0, 0)                  # (2) before (4)
        cross("rb == ra", g, st, a, None, 1, 2, 65, 2, 0, 0)                 # (3) before (4)
        cross("LSR_RING_GRAM_MAX_VECTORS", g, st, a, b, 1, 65, 2, 65537, 0, 0)
        cross("LSR_RING_DOT_MAX_TERMS", g, st, a, b, 1, 2, 2, 65537, h + 1, 0)
        cross("overflow", g, st, a, b, 2**61, 2, 2, 2, h + 1, 0)
        cross("above floor(q / 2)", a, st, a, b, 1, 2, 2, 2, h + 1, 0)       # (7) before the overlap ...
        cross("above floor(q / 2)", a, st, a, b, 0, 2, 2, 2, 0, h + 1)       # ... and before the empty call
        assert lib.lsr_ring_mod_gram_batch_device(ring.handle, a, st, a, b, 0, 2, 2, 2, h, h, None) == 0
        cross("LSR_RING_GRAM_MAX_FAMILY_BYTES", a, st, a, b, 1, 64, 64, 65536, 0, 0)      # (9) before the overlap
        cross("g overlaps a", a, st, a, b, 1, 2, 2, 2, 0, 0)
        cross("g overlaps b", b + 8, st, a, b, 1, 2, 2, 2, 0, 0)
        cross("status overlaps a", g, a + 16, a, b, 1, 2, 2, 2, 0, 0)
        cross("status overlaps g", g, g, a, b, 1, 2, 2, 2, 0, 0)
        with pytest.raises(pkg.CoreError, match="above floor"):
            ring.gram(np.zeros((1, 2, 2, n), dtype=np.uint64), bound_a=h + 1)
        assert ring.gram(np.zeros((1, 2, 2, n), dtype=np.uint64), bound_a=h, bound_b=h + 1)[1].tolist() == [1]     # symmetric: bound_b is not read
    with pkg.RingMod(3329, 131072, device=0) as ring:                        # (10): 64 polynomials per prime at the default chunk size
        assert ring._lib.lsr_ring_mod_gram_batch_device(ring.handle, a, st, a, b, 1, 10, 10, 1, 0, 0, None) == -1
        assert "one column at a time" in pkg._abi.last_error()
    q1 = 8246337208321
    with pkg.RingMod(q1, 8, device=0) as ring:                               # (11): P carries one product
        assert ring.max_terms == 1 == pkg.ring_mod_capacity_product(q1, 8, q1 // 2, q1 // 2)
        assert ring._lib.lsr_ring_mod_gram_sym2_batch_device(ring.handle, a, st, a, b, 1, 2, 2, 0, 0, None) == -1
        msg = pkg._abi.last_error()
        assert "cross form" in msg and "lsr_ring_mod_gram_batch" in msg
        assert ring._lib.lsr_ring_mod_gram_sym2_batch_device(ring.handle, a, st, a, b, 1, 2, 2, 1, 1, None) == -1
        assert "overlaps a" in pkg._abi.last_error()
        rng = np.random.default_rng(8)
        x, y = _random(rng, q1, (2, 3, 3, 8)), _random(rng, q1, (2, 3, 3, 8))       # the cross form there: one column a group
        assert _same(_device(torch, ring, x, y), _want(model.gram(x, y, q1), (2, 3, 3, 8)))


# ---- 9. the integer flavour of the prime contexts -------------------------------------------------------------------------------------
_INTEGER_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as entry
pkg = entry.load_package()
pkg._abi.lib().lsr_set_arith_mode(1)          # before any context: every kernel of this process is the integer flavour's
data = np.load(sys.argv[2] + "/in.npz")
a, b, b5 = data["a"], data["b"], data["b5"]
with pkg.RingMod(int(data["q"]), a.shape[-1], device=0) as ring:
    assert not ring.prime_context(0).uses_f64 and not ring.prime_context(1).uses_f64
    out = dict(zip(("cross", "cross_status"), ring.gram(a, b)))
    out.update(zip(("sym", "sym_status"), ring.gram(a)))
    out.update(zip(("sym2", "sym2_status"), ring.gram_sym2(a, b5)))
np.savez(sys.argv[2] + "/out.npz", **out)
"""


def test_integer_flavour_in_a_fresh_process_equals_the_model(pkg, tmp_path):
    """a child process that forces the integer kernels before it creates a handle (the switch test_ring_mod_matvec_gpu.py sets around
    a create): both primes in one launch of the U64 instantiations, in the three modes"""
    import subprocess
    import sys
    n, q = 64, P5
    a, b, b5, want = _parity_reference(n, q)
    np.savez(str(tmp_path / "in.npz"), q=np.uint64(q), a=a, b=b, b5=b5)
    script = tmp_path / "integer_flavour.py"
    script.write_text(_INTEGER_CHILD)
    subprocess.run([sys.executable, str(script), ROOT, str(tmp_path)], check=True, timeout=300)
    out = np.load(str(tmp_path / "out.npz"))
    for form in ("cross", "sym", "sym2"):
        assert _same((out[form], out[form + "_status"]), want[form]), form
