"""GPU suite: the twisted inner product of a ring handle under an arbitrary modulus, c_j = sum_i sigma_g(a_{j,i}) b_{j,i} in
Z_q[X]/(X^n + 1) (RingMod.ring_dot_galois, lsr_ring_mod_dot_galois_batch): every tile log-size LT = 1 .. 12, both
arithmetic flavours and both forms of b (per output: BHAT false; one shared b: BHAT true) of ntt_tile_ring_dot_lift_galois<A, LT, BHAT>,
under the two moduli of test_ring_mod_sweep_gpu.py:
  top   the largest q the handle admits at n: capacity 1, every term is a group of its own and reduced with `accumulate`;
  P5    the largest prime = 5 (mod 8) below 2^32: a call is one group (also 33 terms at n = 64, past the FP64 re-centring period).
The largest admissible q is even at some n and odd at others; the even word q / 2, whose negation the kernel and the materialised
sigma_g(a) carry as integers q apart (§5t), is planted in every operand by ring_mod_model.planted.

The reference is ring_mod_model.negacyclic_dot(ring_galois_model.automorphism(a, g, q, sign), b, q) in Python integers, never another
kernel; g = 1 is also held against RingMod.dot's own reference.  Shapes: batch 4096/n + 3 (a full tile and a ragged one; 2 at
n = 4096), 3 terms, g in {3, 2n - 1} (3 = 2n - 1 at n = 2).  Device outputs are one vector longer than the call needs and come back
with that tail untouched.  The references of one (n, q) are computed once and shared by the two flavours."""
import functools

import numpy as np
import pytest

import ring_galois_model as galois
import ring_mod_model as model

pytestmark = pytest.mark.gpu

P5 = model.prime_5_mod_8_below(1 << 32)
SENTINEL = 0x5A5A5A5A5A5A5A5A
TERMS, LONG_TERMS = 3, 33
NEGACYCLIC = -1


def _modulus(logn, name):
    return model.largest_admissible(1 << logn) if name == "top" else P5


def _batch(logn):
    return 2 if logn == 12 else (4096 >> logn) + 3


def _elements(n):
    return sorted({3, 2 * n - 1})


def _twisted(a, b, g, q):
    """a [batch][terms][n], b [batch or 1][terms][n] -> [batch][n] through the two Python models"""
    a, b = a.tolist(), b.tolist()
    out = []
    for j, terms in enumerate(a):
        sa = [galois.automorphism(x, g, q, NEGACYCLIC) for x in terms]
        out.append(model.negacyclic_dot(sa, b[j if len(b) > 1 else 0], q))
    return np.array(out, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def _reference(logn, name, terms=TERMS, batch=None, elements=None):
    n, q = 1 << logn, _modulus(logn, name)
    h, hp = q // 2, min(q // 2 + 1, q - 1)
    batch = batch or _batch(logn)
    rng = np.random.default_rng(7000 + 100 * logn + terms + (name == "top"))
    a = model.planted(rng, q, (batch, terms, n), {0: h, batch - 1: hp})      # all-h and all-(h + 1) polynomials: the lift's two sides
    b = model.planted(rng, q, (batch, terms, n), {0: h, batch - 1: h})
    want = {g: (_twisted(a, b, g, q), _twisted(a, b[1:2], g, q)) for g in (elements or _elements(n))}
    for arr in (a, b) + tuple(w for pair in want.values() for w in pair):
        arr.setflags(write=False)
    return a, b, want


def _dev(torch, x):
    return torch.from_numpy(np.array(x, dtype=np.uint64, order="C").view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _run(torch, ring, d_a, d_b, batch, terms, b_rows, g, want, what):
    n = ring.n
    d_c = torch.full((batch + 1, n), SENTINEL, dtype=torch.int64, device="cuda")
    ring.ring_dot_galois_device(d_c.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), batch, terms, b_rows, g, stream=_stream(torch))
    torch.cuda.synchronize()
    got = _host(d_c)
    assert np.array_equal(got[:-1], want), what
    assert bool((got[-1] == np.uint64(SENTINEL)).all()), (what, "the words behind the output were written")


def _ring(pkg, lib, q, n, flavour):
    lib.lsr_set_arith_mode(0 if flavour == "f64" else 1)
    try:
        return pkg.RingMod(q, n, device=0)
    finally:
        lib.lsr_set_arith_mode(0)


@pytest.mark.parametrize("logn", range(1, 13))
@pytest.mark.parametrize("name", ["top", "P5"])
@pytest.mark.parametrize("flavour", ["f64", "u64"])
def test_every_tile_size_flavour_modulus_and_b_form(pkg, lib, flavour, name, logn):
    import torch
    n, q = 1 << logn, _modulus(logn, name)
    batch = _batch(logn)
    if name == "top":
        assert model.capacity(q, n) == 1 and model.capacity(q + 1, n) == 0
    a, b, want = _reference(logn, name)
    with _ring(pkg, lib, q, n, flavour) as ring:
        assert ring.prime_context(0).uses_f64 == (flavour == "f64") and ring.max_terms == model.capacity(q, n)
        d_a, d_b = _dev(torch, a), _dev(torch, b)
        for g, (each, shared) in want.items():
            where = (flavour, name, n, g)
            _run(torch, ring, d_a, d_b, batch, TERMS, batch, g, each, (where, "per-output b"))
            _run(torch, ring, d_a, d_b[1], batch, TERMS, 1, g, shared, (where, "shared b"))


@pytest.mark.parametrize("flavour", ["f64", "u64"])
def test_33_terms_past_the_recentring_period(pkg, lib, flavour):
    import torch
    logn, n, batch = 6, 64, 3
    a, b, want = _reference(logn, "P5", LONG_TERMS, batch, (2 * n - 1,))
    with _ring(pkg, lib, P5, n, flavour) as ring:
        d_a, d_b = _dev(torch, a), _dev(torch, b)
        each, shared = want[2 * n - 1]
        _run(torch, ring, d_a, d_b, batch, LONG_TERMS, batch, 2 * n - 1, each, (flavour, "33 terms"))
        _run(torch, ring, d_a, d_b[1], batch, LONG_TERMS, 1, 2 * n - 1, shared, (flavour, "33 terms, shared b"))


@pytest.mark.parametrize("name", ["top", "P5"])
def test_g_equal_one_is_the_plain_inner_product(pkg, name):
    import torch
    logn, n = 5, 32
    q, batch = _modulus(logn, name), _batch(logn)
    a, b, _ = _reference(logn, name)
    plain = np.array([model.negacyclic_dot(a[j].tolist(), b[j].tolist(), q) for j in range(batch)], dtype=np.uint64)
    with pkg.RingMod(q, n, device=0) as ring:
        d_a, d_b = _dev(torch, a), _dev(torch, b)
        _run(torch, ring, d_a, d_b, batch, TERMS, batch, 1, plain, (name, "g = 1"))
        assert np.array_equal(ring.dot(a, b), plain), (name, "ring.dot against the same reference")


@pytest.mark.parametrize("logn,name", [(3, "top"), (8, "P5")])
def test_host_form(pkg, logn, name):
    n, q = 1 << logn, _modulus(logn, name)
    a, b, want = _reference(logn, name)
    with pkg.RingMod(q, n, device=0) as ring:
        for g, (each, shared) in want.items():
            assert np.array_equal(ring.ring_dot_galois(a, b, g), each), (name, n, g)
            assert np.array_equal(ring.ring_dot_galois(a, b[1], g), shared), (name, n, g, "shared b")
        assert np.array_equal(ring.ring_dot_galois(a[0], b[0], 2 * n - 1), want[2 * n - 1][0][0]), "one output: [terms, n] in, [n] out"


def test_graph_capture_straight_after_create(pkg):
    """no eager call first: the workspace exists since create.  One stream, both forms of b in one graph, two replays on fresh inputs."""
    import torch
    n, q = 64, model.largest_admissible(64)
    batch, terms, g = 5, 3, 2 * n - 1                         # capacity 1: three groups, each reduced with accumulate
    rng = np.random.default_rng(41)
    ring = pkg.RingMod(q, n, device=0)
    d_a = torch.zeros((batch, terms, n), dtype=torch.int64, device="cuda")
    d_b = torch.zeros((batch, terms, n), dtype=torch.int64, device="cuda")
    d_c = [torch.empty((batch, n), dtype=torch.int64, device="cuda") for _ in range(2)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ring.ring_dot_galois_device(d_c[0].data_ptr(), d_a.data_ptr(), d_b.data_ptr(), batch, terms, batch, g, stream=_stream(torch))
        ring.ring_dot_galois_device(d_c[1].data_ptr(), d_a.data_ptr(), d_b.data_ptr(), batch, terms, 1, g, stream=_stream(torch))
    for _ in range(2):
        a, b = model.planted(rng, q, (batch, terms, n)), model.planted(rng, q, (batch, terms, n))
        d_a.copy_(_dev(torch, a))
        d_b.copy_(_dev(torch, b))
        graph.replay()
        torch.cuda.synchronize()
        for rows, d in zip((batch, 1), d_c):
            assert np.array_equal(_host(d), _twisted(a, b if rows > 1 else b[:1], g, q)), rows
    ring.close()                               # free while idle


def test_refusals_that_read_the_handle(pkg):
    import torch
    with pkg.RingMod(3329, 256, device=0) as ring:
        d = torch.zeros((3, 2, 256), dtype=torch.int64, device="cuda")
        d_c = torch.zeros((2, 256), dtype=torch.int64, device="cuda")
        with pytest.raises(pkg.CoreError, match="lsr_ring_mod_dot_galois_batch_device: g = 513 is not below 2 n = 512"):
            ring.ring_dot_galois_device(d_c.data_ptr(), d.data_ptr(), d[1:].data_ptr(), 2, 2, 1, 513, stream=_stream(torch))
        with pytest.raises(pkg.CoreError, match="overlaps"):
            ring.ring_dot_galois_device(d.data_ptr(), d.data_ptr(), d[1:].data_ptr(), 1, 2, 1, 3, stream=_stream(torch))
    with pkg.RingMod(3329, 8192, device=0) as ring:
        x = np.zeros((1, 1, 8192), dtype=np.uint64)
        with pytest.raises(pkg.CoreError, match="above 4096") as err:
            ring.ring_dot_galois(x, x, 3)
        for word in ("lsr_ring_mod_lift_batch_device", "lsr_ntt_ring_dot_galois_batch_device", "lsr_ring_mod_prime_context",
                     "lsr_ring_mod_reduce_batch_device"):
            assert word in str(err.value), word
