"""GPU suite: the adjoint Pi^T w of the seeded projection (lsr_ntt_ring_project_adjoint_batch and its _device form)
word for word against the Python-integer model of tests/ring_backproject_model.py, in the host and the device form, on every kind of
context; against the library's own project_matrix, automorphism, projection and inner products; with planted weights (all q - 1, a
word = q, 2^64 - 1); in the refusals that read the context; and under graph capture with no warm-up call."""
import numpy as np
import pytest

import ring_backproject_model as model
from ring_backproject_model import ROWS, key_from_bytes, key_from_seed
from test_ring_matvec_gpu import _flavour_context

pytestmark = pytest.mark.gpu

Q14 = 12289
Q44 = 17592180539393           # 44-bit prime, 2^18 | q - 1: every n up to 2^17
Q60 = 1152921504606584833
GOLD = 18446744069414584321
# (n, width): less than one stream word; len 40 crosses a word and ends inside one; one whole block plus a ragged one, four elements
# per block; an element is exactly a block; an element spans four blocks; sixteen blocks per element
SHAPES = [(2, 1), (8, 5), (64, 5), (256, 3), (1024, 5), (4096, 2)]
CONTEXTS = ["q14", "f64", "u64_q44", "u64_q60", "gold"]
SETS = [1, 3, 5, 16]           # below, (for a block of 4) not a multiple of, above and several times the register block of sets
PATTERN = 0x5A5A5A5A5A5A5A5A   # the device outputs before the call: an unwritten word shows


def _context(pkg, lib, kind, n):
    if kind == "q14":
        return Q14, pkg.NttContext(Q14, n, device=0)
    if kind == "gold":
        return GOLD, pkg.CyclicNtt(n)
    return _flavour_context(pkg, lib, kind, n)


def _dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()


def _keys_array(keys):
    return np.array(keys, dtype=np.uint64)


def _weights(rng, q, groups, sets):
    return rng.integers(0, q, size=(groups, sets, ROWS), dtype=np.uint64)


def _device_call(ctx, weights, count, width, conjugate, karr, components, index_base):
    """The device form on outputs pre-filled with PATTERN (status: 7) -> (out uint64 [count, sets, width, n], status list)."""
    import torch
    sets = weights.shape[1]
    d_w, d_keys = _dev(torch, weights), _dev(torch, karr)
    d_out = torch.full((count, sets, width, ctx.n), PATTERN, dtype=torch.int64, device="cuda")
    d_status = torch.full((count,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.ring_project_adjoint_device(d_out.data_ptr(), d_status.data_ptr(), d_w.data_ptr(), count, sets, width, conjugate, d_keys.data_ptr(), components,
                                    17, index_base, torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    return d_out.cpu().numpy().view(np.uint64), d_status.cpu().tolist()


def _check_both_forms(ctx, weights, count, width, conjugate, karr, components, index_base, want, want_status):
    got, status = ctx.ring_project_adjoint(weights, width, count, karr, components=components, conjugate=conjugate, index_base=index_base)
    assert got.dtype == np.uint64 and got.shape == want.shape and status.tolist() == want_status
    assert np.array_equal(got, want), ("host", weights.shape[1], conjugate)
    got, status = _device_call(ctx, weights, count, width, conjugate, karr, components, index_base)
    assert status == want_status and np.array_equal(got, want), ("device", weights.shape[1], conjugate)


# ---- 1. word for word against the model ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", CONTEXTS)
@pytest.mark.parametrize("n,width", SHAPES)
def test_matches_the_model(pkg, lib, oracle, kind, n, width):
    """count 5 with components 2: a ragged last group, three keys (the middle one from bytes), index_base != 0; every sets of SETS
    with conjugate 0 and 1, the host and the device form.  The model runs once, for 16 sets: fewer sets are its leading sets.  Q14
    has no ring above n = 2048: there the longest shape keeps its length at n = 2048."""
    if kind == "q14" and n > 2048:
        n, width = 2048, n * width // 2048
    q, ctx = _context(pkg, lib, kind, n)
    cyclic = kind == "gold"
    count, components, index_base = 5, 2, (1 << 40) + 7
    keys = [key_from_seed(width * n + 1), key_from_bytes(bytes(range(7, 39))), key_from_seed(width * n + 2)]
    karr = _keys_array(keys)
    rng = np.random.default_rng(n + width)
    weights = _weights(rng, q, 3, 16)
    want = {c: model.back_project(oracle, q, n, width, weights.tolist(), count, keys, components, 17, index_base, bool(c), cyclic)[0] for c in (0, 1)}
    assert want[0].any() and (n <= 2 or not np.array_equal(want[0], want[1]))
    for sets in SETS:
        w = np.ascontiguousarray(weights[:, :sets])
        for conjugate in (0, 1):
            _check_both_forms(ctx, w, count, width, conjugate, karr, components, index_base, want[conjugate][:, :sets], [1] * count)
    ctx.close()


def test_one_long_element_conjugated(pkg, lib, oracle):
    n = 1 << 16                                                   # 256 blocks of one element: the reversed run spans them all
    q, ctx = _flavour_context(pkg, lib, "f64", n)
    keys = [key_from_seed(16)]
    weights = _weights(np.random.default_rng(16), q, 1, 1)
    want, _ = model.back_project(oracle, q, n, 1, weights.tolist(), 1, keys, 1, 17, 3, True, False)
    _check_both_forms(ctx, weights, 1, 1, 1, _keys_array(keys), 1, 3, want, [1])
    ctx.close()


def test_large_cyclic_context_matches_the_model(pkg, oracle):
    n = 1 << 18                                                   # the smallest n above 2^17
    ctx = pkg.CyclicNtt(n)
    keys = [key_from_seed(18)]
    weights = _weights(np.random.default_rng(18), GOLD, 1, 1)
    for conjugate in (0, 1):
        want, _ = model.back_project(oracle, GOLD, n, 1, weights.tolist(), 1, keys, 1, 17, 5, bool(conjugate), True)
        _check_both_forms(ctx, weights, 1, 1, conjugate, _keys_array(keys), 1, 5, want, [1])
    ctx.close()


# ---- 2. against the library's own calls ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f64", "gold"])
def test_agrees_with_the_projection_the_automorphism_and_the_inner_products(pkg, lib, oracle, kind):
    n, width, index_base = 256, 3, 9
    q, ctx = _context(pkg, lib, kind, n)
    g = ctx.galois_conjugation
    assert g == (n - 1 if kind == "gold" else 2 * n - 1)
    key = _keys_array([key_from_seed(n + 44)])
    # a unit weight gives the row of the matrix
    for r in (0, 31, 255):
        e = np.zeros((1, 1, ROWS), dtype=np.uint64)
        e[0, 0, r] = 1
        out, status = ctx.ring_project_adjoint(e, width, 1, key, index_base=index_base)
        assert status.tolist() == [1]
        assert np.array_equal(out[0, 0], ctx.ring_project_matrix(key, width, r, 1, index_base=index_base)[0]), r
    # the conjugated output is the automorphism of the plain one
    rng = np.random.default_rng(n)
    weights = _weights(rng, q, 1, 3)
    plain, _ = ctx.ring_project_adjoint(weights, width, 1, key, index_base=index_base)
    conj, _ = ctx.ring_project_adjoint(weights, width, 1, key, conjugate=True, index_base=index_base)
    assert np.array_equal(conj, ctx.ring_automorphism(plain, g)) and not np.array_equal(conj, plain)
    # <sigma_-1(Pi^T w), s> has the constant coefficient <w, Pi s> mod q
    bound = 1 << 20
    s = np.array(rng.integers(-bound, bound + 1, size=(1, width, n), dtype=np.int64).astype(object) % q, dtype=np.uint64)
    p, p_status = ctx.ring_project(s, bound, key, index_base=index_base)
    assert p_status.tolist() == [1] and p.any()
    for k in range(3):
        want = sum(int(w) * int(v) for w, v in zip(weights[0, k].tolist(), p[0].tolist())) % q
        assert int(ctx.ring_dot(conj[0, k], s[0])[0]) == want, k
        assert int(ctx.ring_dot_galois(plain[0, k], s[0], g)[0]) == want, k
    ctx.close()


# ---- 3. planted cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u64_q60", "gold"])
def test_all_weights_q_minus_1(pkg, lib, oracle, kind):
    """Sums of 256 (q - 1): past 64 bits at both moduli, which an accumulator that is too narrow does not survive."""
    n, width, count = 64, 5, 2
    q, ctx = _context(pkg, lib, kind, n)
    keys = [key_from_seed(60)]
    weights = np.full((1, 3, ROWS), q - 1, dtype=np.uint64)
    for conjugate in (0, 1):
        want, _ = model.back_project(oracle, q, n, width, weights.tolist(), count, keys, 2, 17, 0, bool(conjugate), kind == "gold")
        _check_both_forms(ctx, weights, count, width, conjugate, _keys_array(keys), 2, 0, want, [1, 1])
    ctx.close()


@pytest.mark.parametrize("kind,bad", [("f64", None), ("u64_q60", None), ("gold", None), ("gold", 2**64 - 1)])
def test_a_weight_not_below_q_refuses_its_group_only(pkg, lib, oracle, kind, bad):
    """A weight = q (Goldilocks: also 2^64 - 1) in set 2 of group 1 only: status -1 and zeros for exactly that group's vectors."""
    n, width, count, sets = 64, 5, 5, 3
    q, ctx = _context(pkg, lib, kind, n)
    keys = [key_from_seed(5), key_from_seed(6), key_from_seed(7)]
    weights = _weights(np.random.default_rng(5), q, 3, sets)
    weights[1, 2, 200] = q if bad is None else bad
    for conjugate in (0, 1):
        want, want_status = model.back_project(oracle, q, n, width, weights.tolist(), count, keys, 2, 17, 0, bool(conjugate), kind == "gold")
        assert want_status.tolist() == [1, 1, -1, -1, 1] and not want[2:4].any() and want[0].any() and want[1].any() and want[4].any()
        _check_both_forms(ctx, weights, count, width, conjugate, _keys_array(keys), 2, 0, want, want_status.tolist())
    ctx.close()


# ---- 4. the refusals that read the context ---------------------------------------------------------------------------------------------
def test_context_rules_are_refused(pkg):
    n = 4096
    ctx = pkg.NttContext(Q44, n, device=0)
    lib, name = ctx._lib, "lsr_ntt_ring_project_adjoint_batch"
    key = _keys_array([key_from_seed(1)])
    weights = np.zeros((1, 2, ROWS), dtype=np.uint64)
    out = np.zeros((1, 2, 1, n), dtype=np.uint64)
    status = np.zeros(1, dtype=np.int32)

    def call(o, st, count, sets, width, components=1, index_base=0):
        return lib.lsr_ntt_ring_project_adjoint_batch(ctx.handle, o, st, weights.ctypes.data, count, sets, width, 0, key.ctypes.data, components, 17,
                                                      index_base)
    for count, width, components, index_base, needle in [
            (1, (1 << 20) + 1, 1, 0, "2^32"),                     # width n above 2^32
            (1, 1, 1, 2**64 - 256, "index_base"),                 # index_base + 256 wraps
            (1, 1, 2**56, 0, "index_base"),                       # 256 * components wraps
            (1 << 48, 1, 1, 0, "overflow")]:                      # count * sets * 16 fits, * n * 8 does not
        assert call(out.ctypes.data, status.ctypes.data, count, 2, width, components, index_base) == -1
        msg = pkg._abi.last_error()
        assert needle in msg and name + ":" in msg, msg
    # the outputs may not share memory with the weights
    assert call(weights.ctypes.data, status.ctypes.data, 1, 2, 1) == -1
    assert "out overlaps weights" in pkg._abi.last_error() and name + ":" in pkg._abi.last_error()
    assert call(out.ctypes.data, weights.ctypes.data + 2048, 1, 2, 1) == -1
    assert "status overlaps weights" in pkg._abi.last_error()
    assert call(out.ctypes.data, status.ctypes.data, 1, 2, 1, 1, 2**64 - 257) == 0 and status.tolist() == [1]      # the last index that fits
    ctx.close()


# ---- 5. graph capture with no warm-up call ---------------------------------------------------------------------------------------------
def test_graph_capture_from_the_first_call(pkg, oracle):
    """The first call this context ever sees is the captured one: one kernel on one stream; one replay equals the eager result."""
    import torch
    q, n, width, count, sets = Q44, 1024, 5, 3, 3
    ctx = pkg.NttContext(q, n, device=0)
    keys = _keys_array([key_from_seed(71), key_from_seed(72)])
    weights = _weights(np.random.default_rng(1024), q, 2, sets)
    d_keys, d_w = _dev(torch, keys), _dev(torch, weights)
    d_out = torch.full((count, sets, width, n), PATTERN, dtype=torch.int64, device="cuda")
    d_status = torch.full((count,), 7, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ctx.ring_project_adjoint_device(d_out.data_ptr(), d_status.data_ptr(), d_w.data_ptr(), count, sets, width, 1, d_keys.data_ptr(), 2, 17, 3,
                                        torch.cuda.current_stream().cuda_stream)
    graph.replay()
    torch.cuda.synchronize()
    eager, eager_status = ctx.ring_project_adjoint(weights, width, count, keys, components=2, conjugate=True, index_base=3)
    assert eager_status.tolist() == [1, 1, 1] and d_status.cpu().tolist() == [1, 1, 1]
    assert np.array_equal(d_out.cpu().numpy().view(np.uint64), eager)
    want, _ = model.back_project(oracle, q, n, width, weights.tolist(), count, keys.tolist(), 2, 17, 3, True, False)
    assert np.array_equal(eager, want)
    ctx.close()
