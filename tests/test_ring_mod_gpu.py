"""GPU suite: ring products under an arbitrary modulus (RingMod: lsr_ring_mod_*, batch.h) against the Python-integer
model (tests/ring_mod_model.py), against the library's own single-prime ring inner product where q happens to be an NTT prime, at
the capacity edge in closed form, the two streaming kernels alone, the composed route through the prime contexts, and under graph
capture straight after create.  Every comparison is exact, word for word.  Shapes are the smallest at which each mechanism can fail:
n = 2 and 4 (many outputs per tile), batch 5 (a partial last tile below n = 4096), 33 terms (past the FP64 re-centring period of 32),
n = 4096 (one output per tile), terms above max_terms (groups reduced with accumulate)."""
import functools

import numpy as np
import pytest

import ring_mod_model as model

pytestmark = pytest.mark.gpu

P5 = model.prime_5_mod_8_below(1 << 32)
Q40 = (1 << 40) + 15                       # odd, 41 bits: max_terms is a handful at n = 64
Q40_ODD = (1 << 40) - 87                 # 40 bits, odd
TERMS = [1, 3, 33]
BATCH = 5


def _dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.uint64)).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _random(rng, q, shape):
    return rng.integers(0, q, size=shape, dtype=np.uint64)


def _dot_device(torch, ring, a, b):
    """dot_device on numpy operands a [batch][terms][n], b [b_rows][terms][n]"""
    batch, terms, n = a.shape
    d_a, d_b = _dev(torch, a), _dev(torch, b)
    d_c = torch.full((batch, n), -1, dtype=torch.int64, device="cuda")
    ring.dot_device(d_c.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), batch, terms, b.shape[0], stream=_stream(torch))
    torch.cuda.synchronize()
    return _host(d_c)


@functools.lru_cache(maxsize=None)
def _reference(n, q):
    """operands of the longest sum and the model's sums of their first 1, 3 and 33 terms, for both forms of b: computed once"""
    rng = np.random.default_rng(1000 * n + q % 997)
    a, b = _random(rng, q, (BATCH, max(TERMS), n)), _random(rng, q, (BATCH, max(TERMS), n))
    a[0, 0, :], b[0, 0, :] = q // 2, q // 2                                  # the centred extremes meet
    a[1, 0, :], b[1, 0, :] = min(q // 2 + 1, q - 1), q - 1
    want = {(t, rows): np.array([model.negacyclic_dot(a[j, :t].tolist(), b[j if rows > 1 else 0, :t].tolist(), q) for j in range(BATCH)], dtype=np.uint64)
            for t in TERMS for rows in (1, BATCH)}
    return a, b, want


@pytest.mark.parametrize("n,q", [(2, 2), (4, 3329), (64, P5), (64, 1 << 32), (256, 3329), (256, 1 << 23)])
def test_mul_and_dot_equal_the_model(pkg, n, q):
    import torch
    a, b, want = _reference(n, q)
    with pkg.RingMod(q, n, device=0) as ring:
        assert ring.max_terms == model.capacity(q, n) and ring.primes == model.primes(n)
        for terms in TERMS:
            for rows in (1, BATCH):
                at, bt = np.ascontiguousarray(a[:, :terms]), np.ascontiguousarray(b[:rows, :terms])
                assert np.array_equal(_dot_device(torch, ring, at, bt), want[terms, rows]), (terms, rows)
                assert np.array_equal(ring.dot(at, bt), want[terms, rows]), (terms, rows)
        for rows in (1, BATCH):                                                  # mul: host form, device form, and in place over a
            a1, b1 = np.ascontiguousarray(a[:, 0]), np.ascontiguousarray(b[:rows, 0])
            assert np.array_equal(ring.mul(a1, b1), want[1, rows])
            d_a, d_b = _dev(torch, a1), _dev(torch, b1)
            ring.mul_device(d_a.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), BATCH, rows, stream=_stream(torch))
            torch.cuda.synchronize()
            assert np.array_equal(_host(d_a), want[1, rows])


def test_n_4096_on_sampled_coefficients(pkg):
    import torch
    n, q, terms, batch = 4096, 1 << 32, 2, 3
    rng = np.random.default_rng(4096)
    a, b = _random(rng, q, (batch, terms, n)), _random(rng, q, (batch, terms, n))
    positions = sorted({0, 1, n // 2, n - 2, n - 1} | set(rng.integers(0, n, size=59).tolist()))
    with pkg.RingMod(q, n, device=0) as ring:
        for rows in (batch, 1):
            got = _dot_device(torch, ring, a, b[:rows])
            for j in range(batch):
                at, bt = a[j].tolist(), b[j if rows > 1 else 0].tolist()
                assert [int(got[j, k]) for k in positions] == [model.dot_coefficient(at, bt, q, k) for k in positions], (rows, j)


def _ntt_prime_for(n):
    """p1 of degree n where the handle admits it, else the largest prime = 1 (mod 2n) it admits"""
    p1 = model.primes(n)[0]
    if model.capacity(p1, n) >= 1:
        return p1
    cand = (model.largest_admissible(n) - 1) // (2 * n) * (2 * n) + 1
    while not model.is_prime(cand):
        cand -= 2 * n
    return cand


@pytest.mark.parametrize("n", [64, 4096])
def test_dot_equals_the_single_prime_inner_product_at_an_ntt_prime(pkg, n):
    import torch
    q, terms, batch = _ntt_prime_for(n), 4, 7
    assert model.capacity(q, n) >= 1 and q % (2 * n) == 1
    rng = np.random.default_rng(n + 7)
    a, b = _random(rng, q, (batch, terms, n)), _random(rng, q, (batch, terms, n))
    with pkg.RingMod(q, n, device=0) as ring, pkg.NttContext(q, n, device=0) as ctx:
        for rows in (batch, 1):
            d_a, d_b = _dev(torch, a), _dev(torch, b[:rows])
            d_c = torch.zeros((batch, n), dtype=torch.int64, device="cuda")
            ctx.ring_dot_device(d_c.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), batch, terms, rows, stream=_stream(torch))
            torch.cuda.synchronize()
            assert np.array_equal(_dot_device(torch, ring, a, b[:rows]), _host(d_c)), rows


def test_the_capacity_edge_in_closed_form(pkg):
    """every operand word at centred magnitude h: coefficient n - 1 of a product of two all-(+h) elements is n h^2 — no wrapped term
    there — so `terms` products reach terms n h^2 exactly; with b = all -h it is the negative.  Coefficient k is (2 (k + 1) - n) h^2."""
    import torch
    n, q = 64, Q40
    h = q // 2
    cap = model.capacity(q, n)
    assert 2 <= cap <= 16
    p1, p2 = model.primes(n)
    assert cap * n * h * h <= (p1 * p2 - 1) // 2 < (cap + 1) * n * h * h
    with pkg.RingMod(q, n, device=0) as ring:
        assert ring.max_terms == cap
        for terms in (cap, cap + 1, 2 * cap + 1):
            a = np.full((2, terms, n), h, dtype=np.uint64)
            b = np.full((2, terms, n), h, dtype=np.uint64)
            b[1] = q - h                                                          # -h (q is odd)
            want = np.array([[sign * terms * (2 * (k + 1) - n) * h * h % q for k in range(n)] for sign in (1, -1)], dtype=np.uint64)
            assert np.array_equal(_dot_device(torch, ring, a, b), want), terms
            assert np.array_equal(_dot_device(torch, ring, a[:, :, :], b[:1]), np.stack([want[0], want[0]])), terms
            assert np.array_equal(ring.dot(a, b), want), terms


@pytest.mark.parametrize("q", [3329, 1 << 32])
def test_lift_alone(pkg, q):
    import torch
    n, h = 64, q // 2
    x = np.array([0, 1, h, h + 1, q - 1, h - 1, 2, q - 2], dtype=np.uint64)
    with pkg.RingMod(q, n, device=0) as ring:
        for i, p in enumerate(ring.primes):
            want = np.array([model.lift(int(v), q, p) for v in x], dtype=np.uint64)
            d_x, d_out = _dev(torch, x), torch.full((len(x),), -1, dtype=torch.int64, device="cuda")
            ring.lift_device(i, d_out.data_ptr(), d_x.data_ptr(), len(x), stream=_stream(torch))
            ring.lift_device(i, d_x.data_ptr(), d_x.data_ptr(), len(x), stream=_stream(torch))       # in place
            torch.cuda.synchronize()
            assert np.array_equal(_host(d_out), want) and np.array_equal(_host(d_x), want), i


@pytest.mark.parametrize("q", [2, 1 << 32, Q40_ODD])
def test_reduce_alone(pkg, q):
    import torch
    n = 64
    p1, p2 = model.primes(n)
    half = (p1 * p2 - 1) // 2
    rng = np.random.default_rng(q % 1009)
    values = [0, 1, -1, half, -half, half - 1, -(half - 1), q, -q] + [int(v) for v in rng.integers(-2**62, 2**62, size=9)] \
        + [int(rng.integers(0, 2**62)) * int(rng.integers(0, 2**24)) - half // 2 for _ in range(9)]
    assert all(-half <= v <= half for v in values)
    r0 = np.array([v % p1 for v in values], dtype=np.uint64)
    r1 = np.array([v % p2 for v in values], dtype=np.uint64)
    want = np.array([model.reduce(int(x), int(y), q, p1, p2) for x, y in zip(r0, r1)], dtype=np.uint64)
    assert want.tolist() == [v % q for v in values]
    old = _random(rng, q, len(values))
    with pkg.RingMod(q, n, device=0) as ring:
        d_r0, d_r1 = _dev(torch, r0), _dev(torch, r1)
        d_out, d_acc = torch.full((len(values),), -1, dtype=torch.int64, device="cuda"), _dev(torch, old)
        ring.reduce_device(d_out.data_ptr(), d_r0.data_ptr(), d_r1.data_ptr(), len(values), stream=_stream(torch))
        ring.reduce_device(d_acc.data_ptr(), d_r0.data_ptr(), d_r1.data_ptr(), len(values), accumulate=True, stream=_stream(torch))
        torch.cuda.synchronize()
        assert np.array_equal(_host(d_out), want)
        assert _host(d_acc).tolist() == [(int(o) + int(w)) % q for o, w in zip(old, want)]


def test_streaming_kernels_off_the_vector_alignment(pkg):
    """13 words starting one word into the allocations: 8-byte but not 16-byte aligned, and no multiple of the two words of a lane;
    the words around the range stay untouched"""
    import torch
    n, q, count = 64, Q40, 13
    p1, p2 = model.primes(n)
    rng = np.random.default_rng(13)
    x = _random(rng, q, count)
    with pkg.RingMod(q, n, device=0) as ring:
        for offset, words in [(1, count), (0, count), (1, count + 1)]:
            x = _random(rng, q, words)
            d_x = torch.zeros(words + 2, dtype=torch.int64, device="cuda")
            d_x[offset:offset + words].copy_(_dev(torch, x))
            d_r = [torch.full((words + 2,), -1, dtype=torch.int64, device="cuda") for _ in range(2)]
            d_out = torch.full((words + 2,), -1, dtype=torch.int64, device="cuda")
            for i in range(2):
                ring.lift_device(i, d_r[i].data_ptr() + 8 * offset, d_x.data_ptr() + 8 * offset, words, stream=_stream(torch))
            ring.reduce_device(d_out.data_ptr() + 8 * offset, d_r[0].data_ptr() + 8 * offset, d_r[1].data_ptr() + 8 * offset, words, stream=_stream(torch))
            torch.cuda.synchronize()
            for i, p in enumerate((p1, p2)):
                got = _host(d_r[i])
                assert got[offset:offset + words].tolist() == [model.lift(int(v), q, p) for v in x], (offset, words, i)
                assert (got[:offset] == 2**64 - 1).all() and (got[offset + words:] == 2**64 - 1).all()
            got = _host(d_out)
            assert np.array_equal(got[offset:offset + words], x), (offset, words)                 # reduce(lift(x)) = x
            assert (got[:offset] == 2**64 - 1).all() and (got[offset + words:] == 2**64 - 1).all()


def test_streaming_kernels_above_the_fused_limit(pkg):
    import torch
    n, q = 65536, 1 << 32
    rng = np.random.default_rng(65536)
    with pkg.RingMod(q, n, device=0) as ring:
        p1, p2 = ring.primes
        assert (p1, p2) == model.primes(n) and ring.max_terms == model.capacity(q, n)
        for count in (2, 2 * n):
            x = _random(rng, q, count)
            x[:2] = [q // 2, q // 2 + 1]
            d_x = _dev(torch, x)
            d_r = [torch.empty(count, dtype=torch.int64, device="cuda") for _ in range(2)]
            for i in range(2):
                ring.lift_device(i, d_r[i].data_ptr(), d_x.data_ptr(), count, stream=_stream(torch))
            d_out = torch.empty(count, dtype=torch.int64, device="cuda")
            ring.reduce_device(d_out.data_ptr(), d_r[0].data_ptr(), d_r[1].data_ptr(), count, stream=_stream(torch))
            torch.cuda.synchronize()
            assert _host(d_r[0])[:64].tolist() == [model.lift(int(v), q, p1) for v in x[:64]]
            assert _host(d_r[1])[:64].tolist() == [model.lift(int(v), q, p2) for v in x[:64]]
            assert np.array_equal(_host(d_out), x)
        d = torch.zeros(3 * n, dtype=torch.int64, device="cuda")
        for name, args in [("lsr_ring_mod_dot_batch_device", (1, 1, 1, None)), ("lsr_ring_mod_mul_batch_device", (1, 1, None))]:
            assert getattr(ring._lib, name)(ring.handle, d.data_ptr(), d.data_ptr() + 8 * n, d.data_ptr() + 16 * n, *args) == -1
            msg = pkg._abi.last_error()
            assert "4096" in msg and "lsr_ring_mod_lift_batch_device" in msg and "lsr_ring_mod_reduce_batch_device" in msg, msg


def test_composition_with_the_fold_of_the_prime_contexts(pkg):
    """lift -> lsr_ntt_ring_fold_batch_device on each prime context -> reduce: the public contract that puts the rest of the toolkit
    under q"""
    import torch
    n, q, outputs, terms, width = 64, 3329, 3, 4, 2
    rng = np.random.default_rng(64)
    v, p = _random(rng, q, (terms, width, n)), _random(rng, q, (outputs, terms, n))
    want = np.array(model.fold(v.tolist(), p.tolist(), q), dtype=np.uint64)               # [outputs][width][n]
    with pkg.RingMod(q, n, device=0) as ring:
        assert terms <= ring.max_terms
        d_v, d_p = _dev(torch, v), _dev(torch, p)
        d_res = []
        for i in range(2):
            ctx = ring.prime_context(i)
            assert ctx.q == ring.primes[i] and ctx.n == n
            d_vi, d_pi = torch.empty_like(d_v), torch.empty_like(d_p)
            ring.lift_device(i, d_vi.data_ptr(), d_v.data_ptr(), v.size, stream=_stream(torch))
            ring.lift_device(i, d_pi.data_ptr(), d_p.data_ptr(), p.size, stream=_stream(torch))
            d_out = torch.empty((outputs, width, n), dtype=torch.int64, device="cuda")
            ctx.ring_fold_device(d_out.data_ptr(), d_vi.data_ptr(), d_pi.data_ptr(), outputs, terms, 0, width, stream=_stream(torch))
            d_res.append(d_out)
        d_c = torch.empty((outputs, width, n), dtype=torch.int64, device="cuda")
        ring.reduce_device(d_c.data_ptr(), d_res[0].data_ptr(), d_res[1].data_ptr(), outputs * width * n, stream=_stream(torch))
        torch.cuda.synchronize()
        assert np.array_equal(_host(d_c), want)


def test_graph_capture_straight_after_create(pkg):
    """no eager call first: the workspace exists since create.  Both forms of b in one graph; two replays on fresh inputs."""
    import torch
    n, q, batch, terms = 64, Q40, 5, 2 * model.capacity(Q40, 64) + 1
    rng = np.random.default_rng(99)
    ring = pkg.RingMod(q, n, device=0)
    d_a = torch.zeros((batch, terms, n), dtype=torch.int64, device="cuda")
    d_b = torch.zeros((batch, terms, n), dtype=torch.int64, device="cuda")
    d_c = [torch.empty((batch, n), dtype=torch.int64, device="cuda") for _ in range(2)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ring.dot_device(d_c[0].data_ptr(), d_a.data_ptr(), d_b.data_ptr(), batch, terms, batch, stream=torch.cuda.current_stream().cuda_stream)
        ring.dot_device(d_c[1].data_ptr(), d_a.data_ptr(), d_b.data_ptr(), batch, terms, 1, stream=torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        a, b = _random(rng, q, (batch, terms, n)), _random(rng, q, (batch, terms, n))
        d_a.copy_(_dev(torch, a))
        d_b.copy_(_dev(torch, b))
        graph.replay()
        torch.cuda.synchronize()
        for rows, d in zip((batch, 1), d_c):
            want = [model.negacyclic_dot(a[j].tolist(), b[j if rows > 1 else 0].tolist(), q) for j in range(batch)]
            assert _host(d).tolist() == want, rows
    ring.close()                               # free while idle
