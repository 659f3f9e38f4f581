"""GPU suite: the batched ring multiply c = a b in Z_q[X]/(X^n + 1) (and mod X^n - 1 on cyclic contexts), lsr_ntt_ring_mul_batch(_device).
Pinned three ways: a schoolbook negacyclic convolution (independent of the oracle), the ring's own X^k rotation, and the oracle's
composition INTT(NTT(a) . NTT(b)) at every degree 2^1 .. 2^17, in each arithmetic flavour."""
import numpy as np
import pytest

import prover_replay

pytestmark = pytest.mark.gpu

Q44 = 17592180539393           # 44-bit prime, 2^18 | q - 1: every n up to 2^17 (FP64 kernels)
Q_NORTH = 17592169062401       # north_star's prime (n <= 4096)
Q16 = 17592182243329           # the n = 2^16 commitment prime
Q60 = 1152921504606584833      # 60-bit prime (u64 Shoup kernels)
GOLD = 18446744069414584321


def _oracle_ring_mul(oracle, q, n, a, b):
    return oracle.ntt_inverse(q, n, oracle.mul_pointwise(q, n, oracle.ntt_forward(q, n, a), oracle.ntt_forward(q, n, b)))


def _schoolbook(a, b, q):
    n = len(a)
    r = [0] * n
    for i, x in enumerate(a):
        if x == 0:
            continue
        for j, y in enumerate(b):
            k = i + j
            if k < n:
                r[k] = (r[k] + x * y) % q
            else:
                r[k - n] = (r[k - n] - x * y) % q
    return r


def _rand(rng, q, shape):
    return rng.integers(0, q, size=shape, dtype=np.uint64)


@pytest.mark.parametrize("q", [12289, Q_NORTH])
@pytest.mark.parametrize("n", [2, 16, 256])
def test_matches_schoolbook(pkg, q, n):
    rng = np.random.default_rng(n + q % 1000)
    ctx = pkg.NttContext(q, n, device=0)
    a, b = _rand(rng, q, (3, n)), _rand(rng, q, (3, n))
    got = ctx.ring_mul(a, b)
    for j in range(3):
        assert got[j].tolist() == _schoolbook([int(x) for x in a[j]], [int(x) for x in b[j]], q), (q, n, j)
    ctx.close()


@pytest.mark.parametrize("logn", range(1, 18))
def test_times_monomial_is_signed_rotation(pkg, logn):
    n, q = 1 << logn, Q44
    rng = np.random.default_rng(logn)
    ctx = pkg.NttContext(q, n, device=0)
    a = _rand(rng, q, n)
    for k in sorted({0, 1, n // 2, n - 1}):
        xk = np.zeros(n, dtype=np.uint64)
        xk[k] = 1
        want = np.roll(a, k).astype(object)
        want[:k] = (q - want[:k]) % q            # wrapped coefficients change sign (X^n = -1)
        assert np.array_equal(ctx.ring_mul(a, xk).astype(object), want), (n, k)
    ctx.close()


def _batch_for(logn):
    return {8: 7, 16: 3, 17: 2}.get(logn, 5 if logn <= 12 else 2)


@pytest.mark.parametrize("flavour", ["f64", "u64_q60", "u64_q44"])
@pytest.mark.parametrize("logn", range(1, 18))
def test_matches_oracle_composition(pkg, oracle, lib, flavour, logn):
    n = 1 << logn
    q = Q60 if flavour == "u64_q60" else Q44
    batch = _batch_for(logn)
    if flavour == "u64_q44":
        lib.lsr_set_arith_mode(1)
    try:
        ctx = pkg.NttContext(q, n, device=0)
    finally:
        lib.lsr_set_arith_mode(0)
    assert ctx.uses_f64 == (flavour == "f64")
    rng = np.random.default_rng(1000 * logn + len(flavour))
    a, b = _rand(rng, q, (batch, n)), _rand(rng, q, (batch, n))
    want = _oracle_ring_mul(oracle, q, n, a, b)
    assert np.array_equal(ctx.ring_mul(a, b), want), (flavour, n)
    # one b for every product
    assert np.array_equal(ctx.ring_mul(a, b[0]), _oracle_ring_mul(oracle, q, n, a, np.tile(b[0], (batch, 1)))), (flavour, n)
    ctx.close()


@pytest.mark.parametrize("q,n", [(Q_NORTH, 4096), (Q16, 65536)])
def test_shared_b_equals_repeated_rows(pkg, q, n):
    import torch
    rng = np.random.default_rng(n)
    batch = 5
    ctx = pkg.NttContext(q, n, device=0)
    a, b = _rand(rng, q, (batch, n)), _rand(rng, q, n)
    d_a = torch.from_numpy(a.view(np.int64)).cuda()
    d_b1 = torch.from_numpy(b.view(np.int64)).cuda()
    d_bn = torch.from_numpy(np.tile(b, (batch, 1)).view(np.int64)).cuda()
    c1, cn = torch.empty_like(d_a), torch.empty_like(d_a)
    s = torch.cuda.current_stream().cuda_stream
    ctx.ring_mul_device(c1.data_ptr(), d_a.data_ptr(), d_b1.data_ptr(), batch, 1, s)
    ctx.ring_mul_device(cn.data_ptr(), d_a.data_ptr(), d_bn.data_ptr(), batch, batch, s)
    torch.cuda.synchronize()
    assert torch.equal(c1, cn)
    ctx.close()


@pytest.mark.parametrize("q,n", [(Q_NORTH, 4096), (Q16, 65536), (Q60, 1024)])
def test_boundary_inputs(pkg, oracle, q, n):
    ctx = pkg.NttContext(q, n, device=0)
    zero = np.zeros((2, n), dtype=np.uint64)
    top = np.full((2, n), q - 1, dtype=np.uint64)
    assert np.array_equal(ctx.ring_mul(zero, top), zero)
    assert np.array_equal(ctx.ring_mul(top, top), _oracle_ring_mul(oracle, q, n, top, top))
    a = _rand(np.random.default_rng(3), q, (2, n))
    assert np.array_equal(ctx.ring_mul(a, a), _oracle_ring_mul(oracle, q, n, a, a))
    ctx.close()


@pytest.mark.parametrize("q,n", [(Q_NORTH, 4096), (Q16, 65536)])
@pytest.mark.parametrize("alias", ["a", "b"])
def test_output_may_alias_an_input(pkg, oracle, q, n, alias):
    import torch
    rng = np.random.default_rng(7)
    batch = 3
    ctx = pkg.NttContext(q, n, device=0)
    a, b = _rand(rng, q, (batch, n)), _rand(rng, q, (batch, n))
    d_a = torch.from_numpy(a.view(np.int64)).cuda()
    d_b = torch.from_numpy(b.view(np.int64)).cuda()
    out = d_a if alias == "a" else d_b
    ctx.ring_mul_device(out.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), batch, batch, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), _oracle_ring_mul(oracle, q, n, a, b))
    ctx.close()


def test_device_api_is_asynchronous_and_ordered_across_streams(pkg, oracle):
    import torch
    q, n, batch = Q16, 65536, 4
    rng = np.random.default_rng(11)
    ctx = pkg.NttContext(q, n, device=0)
    a, b = _rand(rng, q, (2, batch, n)), _rand(rng, q, (2, batch, n))
    d_a = torch.from_numpy(a.view(np.int64)).cuda()
    d_b = torch.from_numpy(b.view(np.int64)).cuda()
    d_c = torch.empty_like(d_a)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    # two calls on one context from two streams: they share the context's workspace, the context orders them
    ctx.ring_mul_device(d_c[0].data_ptr(), d_a[0].data_ptr(), d_b[0].data_ptr(), batch, batch, s1.cuda_stream)
    ctx.ring_mul_device(d_c[1].data_ptr(), d_a[1].data_ptr(), d_b[1].data_ptr(), batch, batch, s2.cuda_stream)
    s1.synchronize()
    s2.synchronize()
    for j in range(2):
        assert np.array_equal(d_c[j].cpu().numpy().view(np.uint64), _oracle_ring_mul(oracle, q, n, a[j], b[j])), j
    ctx.close()


def test_graph_capture_after_eager_warm_up(pkg, oracle):
    import torch
    q, n, batch = Q16, 65536, 3
    rng = np.random.default_rng(12)
    ctx = pkg.NttContext(q, n, device=0)
    a, b = _rand(rng, q, (batch, n)), _rand(rng, q, (batch, n))
    d_a = torch.from_numpy(a.view(np.int64)).cuda()
    d_b = torch.from_numpy(b.view(np.int64)).cuda()
    d_c = torch.empty_like(d_a)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):      # eager warm-up: allocates the workspace
        ctx.ring_mul_device(d_c.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), batch, batch, side.cuda_stream)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ctx.ring_mul_device(d_c.data_ptr(), d_c.data_ptr(), d_b.data_ptr(), batch, batch, torch.cuda.current_stream().cuda_stream)
    d_c.copy_(d_a)
    graph.replay()
    torch.cuda.synchronize()
    want = _oracle_ring_mul(oracle, q, n, a, b)
    assert np.array_equal(d_c.cpu().numpy().view(np.uint64), want)
    graph.replay()                     # c <- c b again
    torch.cuda.synchronize()
    assert np.array_equal(d_c.cpu().numpy().view(np.uint64), _oracle_ring_mul(oracle, q, n, want, b))
    ctx.close()


def test_first_workspace_call_under_capture_is_refused(pkg):
    import torch
    q, n = Q16, 65536
    ctx = pkg.NttContext(q, n, device=0)
    d = torch.zeros((2, n), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    rc = None
    with torch.cuda.graph(graph, stream=side):
        d.add_(0)                      # (keeps the captured graph non-empty)
        rc = ctx._lib.lsr_ntt_ring_mul_batch_device(ctx.handle, d.data_ptr(), d.data_ptr(), d.data_ptr(), 2, 2,
                                                    torch.cuda.current_stream().cuda_stream)
    assert rc == -1
    assert "eager" in pkg._abi.last_error()
    ctx.close()


def test_free_with_ring_multiply_pending(pkg, oracle):
    import torch
    q, n, batch = Q16, 65536, 64
    ctx = pkg.NttContext(q, n, device=0)
    d_a = torch.randint(0, q, (batch, n), dtype=torch.int64, device="cuda")
    d_b = torch.randint(0, q, (batch, n), dtype=torch.int64, device="cuda")
    d_c = torch.empty_like(d_a)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    ctx.ring_mul_device(d_c.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), batch, batch, side.cuda_stream)
    ctx.close()                        # waits for the call, then frees the workspace
    side.synchronize()
    a, b = d_a[:1].cpu().numpy().view(np.uint64), d_b[:1].cpu().numpy().view(np.uint64)
    assert np.array_equal(d_c[:1].cpu().numpy().view(np.uint64), _oracle_ring_mul(oracle, q, n, a, b))


def test_cyclic_context_is_polynomial_multiplication(pkg):
    ntt = pkg.CyclicNtt(2048)
    rng = np.random.default_rng(5)
    a = [int(x) for x in rng.integers(0, GOLD, size=1000, dtype=np.uint64)]
    b = [int(x) for x in rng.integers(0, GOLD, size=1000, dtype=np.uint64)]
    pa = np.zeros(2048, dtype=np.uint64)
    pb = np.zeros(2048, dtype=np.uint64)
    pa[:1000], pb[:1000] = a, b
    want = prover_replay._poly_mul(a, b, GOLD)
    got = ntt.ring_mul(pa, pb)
    assert got[:len(want)].tolist() == want
    assert not got[len(want):].any()
    ntt.close()


def test_cyclic_context_matches_oracle_composition(pkg, oracle):
    n = 4096
    ntt = pkg.CyclicNtt(n)
    omega = ntt.omega
    rng = np.random.default_rng(6)
    a, b = rng.integers(0, GOLD, size=(2, n), dtype=np.uint64), rng.integers(0, GOLD, size=(2, n), dtype=np.uint64)
    got = ntt.ring_mul(a, b)
    for j in range(2):
        fa = oracle.cyclic_forward(a[j], GOLD, omega).astype(object)
        fb = oracle.cyclic_forward(b[j], GOLD, omega).astype(object)
        prod = np.array([int(x) for x in (fa * fb) % GOLD], dtype=np.uint64)
        assert np.array_equal(got[j], oracle.cyclic_inverse(prod, GOLD, omega)), j
    ntt.close()


def test_one_large_batch(pkg, oracle):
    """n = 4096 x 65536 products, device-resident (2 GiB per operand): commutativity, a * 1 = a, sampled rows vs the oracle."""
    import torch
    q, n, batch = Q_NORTH, 4096, 65536
    ctx = pkg.NttContext(q, n, device=0)
    g = torch.Generator(device="cuda")
    g.manual_seed(99)
    d_a = torch.randint(0, q, (batch, n), dtype=torch.int64, device="cuda", generator=g)
    d_b = torch.randint(0, q, (batch, n), dtype=torch.int64, device="cuda", generator=g)
    ab, ba = torch.empty_like(d_a), torch.empty_like(d_a)
    s = torch.cuda.current_stream().cuda_stream
    ctx.ring_mul_device(ab.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), batch, batch, s)
    ctx.ring_mul_device(ba.data_ptr(), d_b.data_ptr(), d_a.data_ptr(), batch, batch, s)
    torch.cuda.synchronize()
    assert torch.equal(ab, ba)
    del ba
    one = torch.zeros(n, dtype=torch.int64, device="cuda")
    one[0] = 1
    ctx.ring_mul_device(d_b.data_ptr(), d_a.data_ptr(), one.data_ptr(), batch, 1, s)   # b <- a * 1
    torch.cuda.synchronize()
    assert torch.equal(d_b, d_a)
    rows = [0, 1, 4095, 32768, batch - 1]
    a = d_a[rows].cpu().numpy().view(np.uint64)
    b = torch.randint(0, q, (len(rows), n), dtype=torch.int64, device="cuda", generator=g)
    del d_b
    c = torch.zeros_like(d_a)
    c[rows] = b
    ctx.ring_mul_device(c.data_ptr(), d_a.data_ptr(), c.data_ptr(), batch, batch, s)   # c <- a * c in place on the b side
    torch.cuda.synchronize()
    want = _oracle_ring_mul(oracle, q, n, a, b.cpu().numpy().view(np.uint64))
    assert np.array_equal(c[rows].cpu().numpy().view(np.uint64), want)
    ctx.close()
