"""GPU suite: every FP64 running sum of the library driven past 2^53 in ONE launch (the table of accumulators).

Each kernel that adds products into a double re-centres the sum every kRingDotF64Period = 32 products and after the last one.  The
tests of "the period" at 31 / 32 / 33 / 65 terms elsewhere check the `|| last` half of that condition; a double holds every integer
below 2^53, so the periodic half changes a word only once a partial sum passes 2^53.  Here every case sums N = 3001 IDENTICAL terms
(each product at a position is the same double every time: the sum walks linearly) through the `_device` entry, at a shape at which
the host code provably hands all of them to one launch — derived in a comment at each case, from the function and the capacity named
there.  Where the host code cannot give one launch 3001 terms (the Gram forms of two vectors and more), the case takes the most it
gives, 2048, and asserts the arithmetic of that limit.

Before it launches, each case takes the evaluation-domain residues of its products from the CPU oracle's transforms and asserts, with
tests/f64_walk_model.py, that at least one position loses a bit under EVERY representative mulmod_f64 may return: the case can tell a
kernel without the periodic re-centre from the real one.  (The seeds are chosen so that at least four positions can; the CPU test at the
bottom holds every plan to that.)  Every output word is then compared with a reference that involves no kernel of the library: N times
the schoolbook product on Python integers (n = 64), for ring handles N times ring_mod_model's exact product.

Shapes: n = 64 (two tile rounds, 64 vectors per tile), two different operand sets per call, at most three rows or outputs."""
import contextlib
import functools

import numpy as np
import pytest

import f64_walk_model as walk
import ring_gadget_model as gadget
import ring_galois_model as galois
import ring_mod_model as mod_model
import ring_tile_model as tile
from f64_walk_model import test_representatives_are_one_or_two, test_the_table_for_q44, test_walk_by_hand  # noqa: F401 (collected here: CPU tests)

N = 3001                        # products per sum: 3001 * q / 2 > 2^54 at a 44-bit q
GRAM_COLUMNS = 2048             # the most columns one Gram launch takes of two vectors (see the Gram cases)
LOGN, DEGREE = 6, 64
Q44 = tile.Q44
P5 = mod_model.prime_5_mod_8_below(1 << 32)
WANTED = 4                      # positions every plan's seed is chosen to reach (the assert before a launch asks for one)
STATUS_SENTINEL = 77
NTT_CHUNK_BYTES = 256 << 20     # ntt_chunk_bytes() with LAMBDA_SNARK_NTT_CHUNK_MIB unset, as the suite runs
RING_WORKSPACE_POLYS = min((NTT_CHUNK_BYTES // 3) >> (LOGN + 3), 4096)      # ring_dot_chunk_polys at n <= 4096 (lsr_ring_workspace.hpp)
assert N * (Q44 // 2) > 2**54 and RING_WORKSPACE_POLYS == 4096 >= N


@pytest.fixture
def opened():
    """opened(handle) -> handle, closed when the case ends, the last opened first — also when an assertion of the case fails, so that
    no handle is left to the garbage collector behind a traceback"""
    with contextlib.ExitStack() as stack:
        def register(handle):
            stack.callback(handle.close)
            return handle
        yield register


# ---- flavours ------------------------------------------------------------------------------------------------------------------------
def _q45(oracle):
    q = int(oracle.L.oracle_largest_prime_1mod(2 * DEGREE, 45))
    assert 2**44 < q < 2**45
    return q


def _flavour(oracle, flavour):
    """(q, cyclic, omega): f64 and cyc_f64 at the 44-bit prime, q45 the largest 45-bit prime = 1 mod 2n (negacyclic)"""
    if flavour == "q45":
        return _q45(oracle), False, 0
    q, cyclic = tile.FLAVOURS[flavour]
    return q, cyclic, tile.omega_for(oracle, flavour, DEGREE)


def _open(pkg, oracle, opened, flavour):
    q, cyclic, omega = _flavour(oracle, flavour)
    ctx = opened(pkg.CyclicNtt(DEGREE, modulus=q, omega=omega) if cyclic else pkg.NttContext(q, DEGREE, device=0))
    lib = pkg._abi.lib()
    assert bool(lib.lsr_ntt_context_uses_f64(ctx.handle)) and lib.lsr_ntt_context_is_cyclic(ctx.handle) == int(cyclic), flavour
    return q, cyclic, omega, ctx


# ---- CPU: residues of the products, the discriminator, the references -------------------------------------------------------------------
def _forward(oracle, q, polys, cyclic=False, omega=0):
    """the oracle's forward transform of polys [..., n] as an object array of Python integers"""
    polys = np.ascontiguousarray(polys, dtype=np.uint64)
    flat = polys.reshape(-1, DEGREE)
    if cyclic:
        out = np.stack([oracle.cyclic_forward(row, q, omega) for row in flat])
    else:
        out = np.asarray(oracle.ntt_forward(q, DEGREE, flat))
    return np.array(out.tolist(), dtype=object).reshape(polys.shape)


def _products(oracle, q, a, b, cyclic=False, omega=0):
    """the residues of NTT(a) . NTT(b), position by position (a and b [..., n], equal shapes) -> object array"""
    return _forward(oracle, q, a, cyclic, omega) * _forward(oracle, q, b, cyclic, omega) % q


def _telling(cycle, q, steps, start=0):
    """how many positions of the walk over the cycle of residue arrays can tell; the arrays are flattened side by side"""
    residues = np.stack([np.asarray(r, dtype=object).reshape(-1) for r in cycle])
    return len(walk.discriminating_positions(residues, q, steps, start))


def _assert_can_tell(count, what):
    assert count >= 1, "%r: no position of this case can tell a lost re-centre (%d positions)" % (what, count)


def _scaled(poly, times, q):
    return [int(v) * times % q for v in poly]


def _rand(rng, q, shape):
    return rng.integers(0, q, size=shape, dtype=np.uint64)


def _repeat(x, axis, times):
    """x with a new axis of `times` identical copies at `axis`, contiguous"""
    return np.ascontiguousarray(np.repeat(np.expand_dims(x, axis), times, axis=axis))


def _dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint64).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _empty(torch, *shape):
    return torch.full(shape, 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")


# ---- plans: the operands of a case and what the model says of them, computed once on the CPU -------------------------------------------
DOT_CASES = [("f64", False, 1), ("f64", True, 2), ("cyc_f64", False, 3), ("cyc_f64", True, 4), ("q45", False, 5), ("q45", True, 6)]
GALOIS_CASES = [("f64", "five", 11), ("f64", "conjugation", 12), ("cyc_f64", "five", 13), ("cyc_f64", "conjugation", 14)]
GRAM_CASES = [("cross", 1, GRAM_COLUMNS, 31), ("sym", 2, GRAM_COLUMNS, 32), ("sym", 1, N, 33), ("sym2", 2, GRAM_COLUMNS // 2, 34)]
SCALAR_CASES = [(flavour, sets, aligned, addend, 40 + i)
                for i, (flavour, sets, aligned, addend) in enumerate((f, s, al, ad) for f in ("f64", "q45") for s in (1, 3) for al in (True, False)
                                                                     for ad in (False, True))]
MOD_CASES = ["dot", "dot_shared", "fold", "matvec", "matvec_bounded", "gram_cross", "galois"]
MOD_BOUND_X = 1 << 20


@functools.lru_cache(maxsize=None)
def _dot_plan(oracle, flavour, shared, seed):
    q, cyclic, omega = _flavour(oracle, flavour)
    rng = np.random.default_rng(seed)
    a0, b0 = _rand(rng, q, (2, DEGREE)), _rand(rng, q, (1 if shared else 2, DEGREE))
    bb = np.broadcast_to(b0, a0.shape)
    count = _telling([_products(oracle, q, a0, bb, cyclic, omega)], q, N)
    want = [_scaled(tile.schoolbook(a0[j], bb[j], q, 1 if cyclic else -1), N, q) for j in range(2)]
    return a0, b0, count, want


@functools.lru_cache(maxsize=None)
def _fold_plan(oracle, seed):
    q, width = Q44, 2
    rng = np.random.default_rng(seed)
    v0, p0 = _rand(rng, q, (2, width, DEGREE)), _rand(rng, q, (2, DEGREE))
    count = _telling([_products(oracle, q, v0, np.broadcast_to(p0[:, None, :], v0.shape))], q, N)
    want = [[_scaled(tile.schoolbook(p0[j], v0[j, c], q, -1), N, q) for c in range(width)] for j in range(2)]
    return v0, p0, count, want


@functools.lru_cache(maxsize=None)
def _galois_plan(oracle, flavour, which, seed):
    q, cyclic, omega = _flavour(oracle, flavour)
    sign = 1 if cyclic else -1
    g = 5 if which == "five" else galois.galois_order(DEGREE, sign) - 1
    rng = np.random.default_rng(seed)
    a0, b0 = _rand(rng, q, (2, DEGREE)), _rand(rng, q, (2, DEGREE))
    sa = galois.automorphism_np(a0, g, q, sign)
    assert sa[0].tolist() == galois.automorphism(a0[0], g, q, sign)
    count = _telling([_products(oracle, q, sa, b0, cyclic, omega)], q, N)
    want = [_scaled(tile.schoolbook(sa[j], b0[j], q, sign), N, q) for j in range(2)]
    return g, a0, b0, count, want


@functools.lru_cache(maxsize=None)
def _matvec_plan(oracle, seed):
    q, rows = Q44, 3
    rng = np.random.default_rng(seed)
    m0, x0 = _rand(rng, q, (rows, DEGREE)), _rand(rng, q, (2, DEGREE))
    pairs_m, pairs_x = np.repeat(m0, 2, axis=0), np.tile(x0, (rows, 1))
    count = _telling([_products(oracle, q, pairs_m, pairs_x)], q, N)
    want = [[_scaled(tile.schoolbook(m0[r], x0[j], q, -1), N, q) for r in range(rows)] for j in range(2)]
    return m0, x0, count, want


GADGET_BASE_LOG2, GADGET_DIGITS = 16, 3


@functools.lru_cache(maxsize=None)
def _gadget_plan(oracle, seed):
    """M holds its polynomial on the digit-0 column of every x column and zeros on the others: N effective columns among N D matrix
    columns, and the products of one x column are the cycle (m z_0, 0, 0), which the walk model takes as it is."""
    q, rows = Q44, 2
    assert gadget.min_digits(q, GADGET_BASE_LOG2) == GADGET_DIGITS == walk.MAX_DISTINCT
    rng = np.random.default_rng(seed)
    m0, x0 = _rand(rng, q, (rows, DEGREE)), _rand(rng, q, (2, DEGREE))
    z0 = gadget.decompose(x0, q, GADGET_BASE_LOG2, GADGET_DIGITS)[:, 0]            # digit 0 of x0[j] as canonical residues [2, n]
    first = _products(oracle, q, np.repeat(m0, 2, axis=0), np.tile(z0, (rows, 1)))
    nothing = np.zeros_like(first)
    count = _telling([first, nothing, nothing], q, N * GADGET_DIGITS)
    want = [[_scaled(tile.schoolbook(m0[r], z0[j], q, -1), N, q) for r in range(rows)] for j in range(2)]
    return m0, x0, count, want


@functools.lru_cache(maxsize=None)
def _gram_plan(oracle, form, r, width, seed):
    """Vector i of family j is the polynomial a0[j][i] in every column.  cross: G[i][l] = width a_i b_l; sym: the packed triangle of
    width a_i a_l; sym2: width (a_i b_l + a_l b_i) off the diagonal — two products per column, the cycle (a_i b_l, a_l b_i) — and
    width a_i b_i on it, which at 1024 columns no position can tell (f64_walk_model.test_the_table_for_q44) and is left out of the count.

    sym2 with two INDEPENDENT families cannot tell anywhere at the 1024 columns one launch takes: among the four choices of
    representatives one has |v1 + v2| <= q / 2, and 1024 such pairs stay below 2^53 (_sym2_independent_families, asserted on the CPU).
    So the sym2 case hands over b = a in a buffer of its own: the two products of a column are then mulmod_f64(a_0, a_1) and
    mulmod_f64(a_1, a_0), the same double — x w and fma(x, w, -h) are symmetric in their operands — and the off-diagonal sum walks
    2048 times over ONE product, whatever its representative."""
    q = Q44
    rng = np.random.default_rng(seed)
    a0, b0 = _rand(rng, q, (2, r, DEGREE)), _rand(rng, q, (2, r, DEGREE))
    if form == "sym2":
        b0 = a0.copy()
    mul = lambda x, y: tile.schoolbook(x, y, q, -1)                                  # noqa: E731
    if form == "cross":
        count = _telling([_products(oracle, q, a0, b0)], q, width)
        want = [[[_scaled(mul(a0[j, i], b0[j, l]), width, q) for l in range(r)] for i in range(r)] for j in range(2)]
    elif form == "sym":
        il = [(i, l) for i in range(r) for l in range(i, r)]
        count = _telling([_products(oracle, q, a0[:, [i for i, _ in il]], a0[:, [l for _, l in il]])], q, width)
        want = [[_scaled(mul(a0[j, i], a0[j, l]), width, q) for i, l in il] for j in range(2)]
    else:
        assert r == 2
        count = _telling([_products(oracle, q, a0[:, 0], a0[:, 1])], q, 2 * width)
        want = []
        for j in range(2):
            cross = [(x + y) % q for x, y in zip(mul(a0[j, 0], b0[j, 1]), mul(a0[j, 1], b0[j, 0]))]
            want.append([_scaled(mul(a0[j, 0], b0[j, 0]), width, q), _scaled(cross, width, q), _scaled(mul(a0[j, 1], b0[j, 1]), width, q)])
    return a0, b0, count, want


def _sym2_independent_families(oracle, seed):
    """how many of 4 * n off-diagonal positions of sym2 with r = 2 and two independent random families can tell at the 1024 columns
    (2048 products, the cycle (a_0 b_1, a_1 b_0)) one launch takes"""
    rng = np.random.default_rng(seed)
    a0, b0 = _rand(rng, Q44, (4, 2, DEGREE)), _rand(rng, Q44, (4, 2, DEGREE))
    return _telling([_products(oracle, Q44, a0[:, 0], b0[:, 1]), _products(oracle, Q44, a0[:, 1], b0[:, 0])], Q44, GRAM_COLUMNS)


@functools.lru_cache(maxsize=None)
def _scalar_plan(oracle, flavour, sets, addend, seed):
    """Output j sums N copies of the vector v0[j] under the weight w0[j][k] of set k: position by position the product v w, no
    transform.  The sum starts at the addend word (canonical: one representative) or at 0."""
    q = _flavour(oracle, flavour)[0]
    rng = np.random.default_rng(seed)
    v0, w0 = _rand(rng, q, (2, DEGREE)), _rand(rng, q, (2, sets))
    add = _rand(rng, q, (2, sets, 1, DEGREE)) if addend else None
    vo, wo = np.array(v0.tolist(), dtype=object), np.array(w0.tolist(), dtype=object)
    residues = (wo[:, :, None] * vo[:, None, :]) % q                                 # [2, sets, n]
    start = 0 if add is None else [int(x) for x in add.reshape(-1)]
    count = _telling([residues], q, N, start)
    total = residues * N + (0 if add is None else np.array(add.tolist(), dtype=object).reshape(2, sets, DEGREE))
    want = np.array((total % q).tolist(), dtype=np.uint64).reshape(2, sets, 1, DEGREE)
    return v0, w0, add, count, want


def _lifted_products(oracle, q, a, b):
    """the products of a ring handle under each of its two primes: the lifted operands transformed under the prime"""
    cycle_free = []
    for p in mod_model.primes(DEGREE):
        la, lb = (np.array([[mod_model.lift(int(w), q, p) for w in row] for row in x.reshape(-1, DEGREE)], dtype=np.uint64).reshape(x.shape) for x in (a, b))
        cycle_free.append((p, _products(oracle, p, la, lb)))
    return cycle_free


def _mod_telling(oracle, q, a, b):
    return sum(_telling([products], p, N) for p, products in _lifted_products(oracle, q, a, b))


def _mod_mul(a, b, q, times=N):
    return _scaled(mod_model.negacyclic_mul(a.tolist(), b.tolist(), q), times, q)


@functools.lru_cache(maxsize=None)
def _mod_plan(oracle, which):
    q = P5
    rng = np.random.default_rng(60 + MOD_CASES.index(which))
    if which in ("dot", "dot_shared", "galois"):
        a0, b0 = _rand(rng, q, (2, DEGREE)), _rand(rng, q, (1 if which == "dot_shared" else 2, DEGREE))
        g = 2 * DEGREE - 1 if which == "galois" else 1
        sa = galois.automorphism_np(a0, g, q, -1) if g != 1 else a0
        bb = np.ascontiguousarray(np.broadcast_to(b0, a0.shape))
        return (g, a0, b0), _mod_telling(oracle, q, sa, bb), [_mod_mul(sa[j], bb[j], q) for j in range(2)]
    if which == "fold":
        v0, p0 = _rand(rng, q, (2, DEGREE)), _rand(rng, q, (1, DEGREE))            # ONE output of width 2 (see the case)
        pp = np.ascontiguousarray(np.broadcast_to(p0, v0.shape))
        return (v0, p0), _mod_telling(oracle, q, v0, pp), [_mod_mul(p0[0], v0[c], q) for c in range(2)]
    if which in ("matvec", "matvec_bounded"):
        rows = 3
        m0 = _rand(rng, q, (rows, DEGREE))
        if which == "matvec":
            x0 = _rand(rng, q, (2, DEGREE))
        else:                                                                       # x within the bound the call asserts, both signs
            small = rng.integers(-MOD_BOUND_X, MOD_BOUND_X + 1, size=(2, DEGREE))
            small[0, :2], small[1, :2] = (MOD_BOUND_X, -MOD_BOUND_X), (-MOD_BOUND_X, MOD_BOUND_X)
            x0 = np.array([[int(v) % q for v in row] for row in small], dtype=np.uint64)
        count = _mod_telling(oracle, q, np.repeat(m0, 2, axis=0), np.tile(x0, (rows, 1)))
        return (m0, x0), count, [[_mod_mul(m0[r], x0[j], q) for r in range(rows)] for j in range(2)]
    assert which == "gram_cross"
    a0, b0 = _rand(rng, q, (2, DEGREE)), _rand(rng, q, (2, DEGREE))
    return (a0, b0), _mod_telling(oracle, q, a0, b0), [_mod_mul(a0[j], b0[j], q) for j in range(2)]


# ---- ring_dot ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("flavour,shared,seed", DOT_CASES)
def test_ring_dot(pkg, oracle, opened, flavour, shared, seed):
    """One launch: at n <= 4096 ring_dot_enqueue (lsr_ring_dot.hip) hands a per-output b to ONE ntt_tile_ring_dot launch over all terms
    (terms <= LSR_RING_DOT_MAX_TERMS = 65536), and takes a shared b (b_rows == 1, batch > 1: the BHAT kernel) in groups of
    ring_dot_chunk_polys = min(256 MiB / 3 / 8 n, 4096) = 4096 >= 3001 b-hat rows: one group."""
    import torch
    a0, b0, count, want = _dot_plan(oracle, flavour, shared, seed)
    _assert_can_tell(count, ("ring_dot", flavour, shared))
    q, _, _, ctx = _open(pkg, oracle, opened, flavour)
    d_a = _dev(torch, _repeat(a0, 1, N))
    d_b = _dev(torch, _repeat(b0[0], 0, N) if shared else _repeat(b0, 1, N))
    d_c = _empty(torch, 2, DEGREE)
    ctx.ring_dot_device(d_c.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), 2, N, 1 if shared else 2, _stream(torch))
    torch.cuda.synchronize()
    assert _host(d_c).tolist() == want, (flavour, shared, count)


# ---- ring_fold --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_ring_fold(pkg, oracle, opened):
    """One launch per output: at n <= 4096 ring_fold_enqueue (lsr_ring_fold.hip) takes whole outputs while terms <=
    ring_dot_chunk_polys = 4096, polys / terms = 1 output per chunk, each ONE ntt_tile_ring_fold launch over its 3001 terms."""
    import torch
    v0, p0, count, want = _fold_plan(oracle, 7)
    _assert_can_tell(count, "ring_fold")
    q, _, _, ctx = _open(pkg, oracle, opened, "f64")
    width = v0.shape[1]
    d_v = _dev(torch, _repeat(v0, 1, N))                 # [2][N][width][n]: term_stride = N, output j reads N copies of v0[j]
    d_p = _dev(torch, _repeat(p0, 1, N))
    d_out = _empty(torch, 2, width, DEGREE)
    ctx.ring_fold_device(d_out.data_ptr(), d_v.data_ptr(), d_p.data_ptr(), 2, N, N, width, _stream(torch))
    torch.cuda.synchronize()
    assert _host(d_out).tolist() == want, count


# ---- ring_dot_galois ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("flavour,which,seed", GALOIS_CASES)
def test_ring_dot_galois(pkg, oracle, opened, flavour, which, seed):
    """One launch: ring_dot_galois_enqueue (lsr_ring_galois.hip) hands a per-output b to ONE ntt_tile_ring_dot_galois launch over all
    terms.  g = 5 and the conjugation g = N - 1; the products are those of sigma_g(a) with b."""
    import torch
    g, a0, b0, count, want = _galois_plan(oracle, flavour, which, seed)
    _assert_can_tell(count, ("ring_dot_galois", flavour, g))
    q, _, _, ctx = _open(pkg, oracle, opened, flavour)
    assert which != "conjugation" or g == ctx.galois_conjugation
    d_a, d_b, d_c = _dev(torch, _repeat(a0, 1, N)), _dev(torch, _repeat(b0, 1, N)), _empty(torch, 2, DEGREE)
    ctx.ring_dot_galois_device(d_c.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), 2, N, 2, g, _stream(torch))
    torch.cuda.synchronize()
    assert _host(d_c).tolist() == want, (flavour, g, count)


# ---- matvec and matvec_gadget -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_matvec(pkg, oracle, opened):
    """One launch: at n <= 4096 matvec_device (lsr_ring_matvec.hip) is ONE ntt_tile_ring_matvec launch over all cols <=
    LSR_RING_DOT_MAX_TERMS columns of the resident matrix."""
    import torch
    m0, x0, count, want = _matvec_plan(oracle, 8)
    _assert_can_tell(count, "matvec")
    q, _, _, ctx = _open(pkg, oracle, opened, "f64")
    rows = m0.shape[0]
    d_m, d_x, d_y = _dev(torch, _repeat(m0, 1, N)), _dev(torch, _repeat(x0, 1, N)), _empty(torch, 2, rows, DEGREE)
    mat = opened(ctx.ring_matrix_device(d_m.data_ptr(), rows, N, _stream(torch)))
    mat.matvec_device(d_y.data_ptr(), d_x.data_ptr(), 2, _stream(torch))
    torch.cuda.synchronize()
    assert _host(d_y).tolist() == want, count


@pytest.mark.gpu
def test_matvec_gadget(pkg, oracle, opened):
    """One launch: matvec_gadget_device is ONE ntt_tile_ring_matvec_gadget launch over all cols = 3001 * 3 = 9003 <=
    LSR_RING_DOT_MAX_TERMS matrix columns.  Its period counts MATRIX columns: the real kernel re-centres after every 10 or 11 of the
    3001 non-zero products."""
    import torch
    m0, x0, count, want = _gadget_plan(oracle, 9)
    _assert_can_tell(count, "matvec_gadget")
    q, _, _, ctx = _open(pkg, oracle, opened, "f64")
    assert pkg.ring_gadget_min_digits(q, GADGET_BASE_LOG2) == GADGET_DIGITS
    rows, cols = m0.shape[0], N * GADGET_DIGITS
    m = np.zeros((rows, cols, DEGREE), dtype=np.uint64)
    m[:, ::GADGET_DIGITS] = m0[:, None, :]
    d_m, d_x, d_y = _dev(torch, m), _dev(torch, _repeat(x0, 1, N)), _empty(torch, 2, rows, DEGREE)
    mat = opened(ctx.ring_matrix_device(d_m.data_ptr(), rows, cols, _stream(torch)))
    mat.matvec_gadget_device(d_y.data_ptr(), d_x.data_ptr(), 2, GADGET_BASE_LOG2, GADGET_DIGITS, _stream(torch))
    torch.cuda.synchronize()
    assert _host(d_y).tolist() == want, count


# ---- Gram -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form,r,width,seed", GRAM_CASES)
def test_ring_gram(pkg, oracle, opened, form, r, width, seed):
    """ring_gram_enqueue (lsr_ring_gram.hip) keeps a family in one launch while vectors * width <= gram_workspace_polys = the ring
    workspace's 4096 polynomials at every n <= 4096, vectors = ra + rb (cross, sym2) or r (sym); beyond that it takes polys / vectors
    columns per launch and hands canonical words over.  So no launch of the cross form, of sym with r = 2 or of sym2 ever sums more
    than 2048 columns (1024 for sym2 with r = 2, two products each), at n > 4096 fewer: 3001 in one launch cannot be reached there, and
    these cases take the 2048 that can, at which the walk model still finds positions (about one in eight).  sym with r = 1 gets all
    3001 columns into one launch.  sym2 is given b = a in a second buffer, the one way its two products per column add up to a walk
    that can tell within 1024 columns (_gram_plan).  Families per launch: polys / (vectors * width) = 1, so family 1 is a second launch of the same kind."""
    import torch
    vectors = r if form == "sym" else 2 * r
    assert vectors * width <= RING_WORKSPACE_POLYS and (width == N or vectors * (width + 1) > RING_WORKSPACE_POLYS)
    a0, b0, count, want = _gram_plan(oracle, form, r, width, seed)
    _assert_can_tell(count, ("ring_gram", form, r, width))
    q, _, _, ctx = _open(pkg, oracle, opened, "f64")
    d_a, d_b = _dev(torch, _repeat(a0, 2, width)), _dev(torch, _repeat(b0, 2, width))          # [2][r][width][n]
    if form == "cross":
        d_g = _empty(torch, 2, r, r, DEGREE)
        ctx.ring_gram_device(d_g.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), 2, r, r, width, _stream(torch))
    elif form == "sym":
        d_g = _empty(torch, 2, r * (r + 1) // 2, DEGREE)
        ctx.ring_gram_device(d_g.data_ptr(), d_a.data_ptr(), None, 2, r, r, width, _stream(torch))
    else:
        d_g = _empty(torch, 2, r * (r + 1) // 2, DEGREE)
        ctx.ring_gram_sym2_device(d_g.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), 2, r, width, _stream(torch))
    torch.cuda.synchronize()
    assert _host(d_g).tolist() == want, (form, r, width, count)


# ---- scalar combine -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("flavour,sets,aligned,addend,seed", SCALAR_CASES)
def test_ring_scalar_combine(pkg, oracle, opened, flavour, sets, aligned, addend, seed):
    """One launch: scalar_combine_device (lsr_ring_scalar.hip) is one ring_scalar_combine_kernel launch per block of sets over all
    terms <= 65536; the kernel stages 128 terms at a time and counts its period from each stage's first term, 3001 = 23 * 128 + 57: the
    last stage is partial.  Buffers off 16-byte alignment take one position per lane (P = 1), aligned ones two."""
    import torch
    v0, w0, add, count, want = _scalar_plan(oracle, flavour, sets, addend, seed)
    _assert_can_tell(count, ("ring_scalar_combine", flavour, sets, aligned, addend))
    q, _, _, ctx = _open(pkg, oracle, opened, flavour)

    def place(x):
        """x on the device at an address that is (aligned) or is not a multiple of 16"""
        flat = np.ascontiguousarray(x, dtype=np.uint64).reshape(-1)
        buf = torch.empty(flat.size + 2, dtype=torch.int64, device="cuda")
        view = buf[(0 if aligned else 1) + (buf.data_ptr() % 16) // 8:][:flat.size]
        view.copy_(torch.from_numpy(flat.view(np.int64)))
        assert (view.data_ptr() % 16 == 0) == aligned
        return view

    d_v = place(_repeat(v0, 1, N))                       # [2][N][1][n]: term_stride = N
    d_w = _dev(torch, _repeat(w0, 2, N))                 # [2 groups][sets][N]
    d_out = place(np.zeros((2, sets, 1, DEGREE), dtype=np.uint64))
    d_add = place(add) if addend else None
    d_status = torch.full((2,), STATUS_SENTINEL, dtype=torch.int32, device="cuda")
    ctx.ring_scalar_combine_device(d_out.data_ptr(), d_status.data_ptr(), d_v.data_ptr(), d_w.data_ptr(), d_add.data_ptr() if addend else None, 2, sets,
                                   N, N, 1, 1, _stream(torch))
    torch.cuda.synchronize()
    assert d_status.cpu().tolist() == [1, 1]
    assert np.array_equal(_host(d_out).reshape(want.shape), want), (flavour, sets, aligned, addend, count)


# ---- ring_combine_rows --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["default", "rns"])
def test_ring_combine_rows(pkg, oracle, opened, kind):
    """One launch per prime: at n <= 4096 ring_combine_rows_device (lsr_commit.hip) takes whole outputs while terms <=
    ring_combine_polys = 256 MiB / 8 n (half of it per prime under RNS) = 524288 (262144) >= 3001: outputs 0 and 1 in one
    ring_combine_tile launch per prime.  The budget: a unit monomial weighs 1, 3001 of them stay within lsr_lwe_combine_max_weight at
    n = 64, k = 1 (asserted).  Output j combines 3001 copies of committed row j with the constant polynomial 1: the products are the
    transformed row components themselves, the body 3001 * row mod q."""
    import torch
    import ring_combine_model as combine
    n, k = DEGREE, 1
    params = pkg.Params(n=n, k=k, sigma=3.19)
    ctx = opened(pkg.LweContext.create_rns(params, key_seed=77) if kind == "rns" else pkg.LweContext(params, key_seed=77))
    assert ctx.combine_max_weight >= N
    moduli = tuple(ctx.rns_moduli() or (ctx.commit_modulus,))
    assert len(moduli) == (2 if kind == "rns" else 1) and all(2**43 < q < 2**44 for q in moduli)
    # the FP64 flavour: read off the context's own NttContext where the ABI lends it; it refuses an RNS context (two transforms), whose
    # members take their flavour by the rule of every NttContext (lsr_ntt.hip: q < 2^45 and the process-wide arithmetic mode at
    # creation), so there a context of each modulus opened next to it is asked
    lib = pkg._abi.lib()
    if kind == "rns":
        assert not lib.lsr_lwe_ntt_context(ctx.handle)
        assert all(opened(pkg.NttContext(q, n, device=0)).uses_f64 for q in moduli)
    else:
        assert lib.lsr_ntt_context_uses_f64(lib.lsr_lwe_ntt_context(ctx.handle))
    rng = np.random.default_rng(90 + len(kind))
    msgs = rng.integers(0, ctx.plain_modulus, size=(2, n), dtype=np.uint64)
    base = np.ascontiguousarray(pkg.Commitment.batch_words(ctx, msgs, np.array([5, 6], dtype=np.uint64)), dtype=np.uint64)
    head, blocks = combine.layout(n, k, moduli)
    assert base.shape == (2, ctx.commitment_words) and ctx.commitment_words == head + len(moduli) * (k + 1) * n
    ones = np.zeros((2, k + 1, n), dtype=np.uint64)
    ones[:, :, 0] = 1
    count = 0
    for first, words, q in blocks:
        comps = base[:, first:first + words].reshape(2, k + 1, n)
        assert int(comps.max()) < q
        count += _telling([_products(oracle, q, comps, ones)], q, N)             # (the transform of 1 is 1 everywhere)
    _assert_can_tell(count, ("ring_combine_rows", kind))
    assert count >= WANTED, (kind, count)                    # (the rows exist on the device only: held to the seeds' count here)
    want = base.copy()
    for first, words, q in blocks:
        want[:, first:first + words] = np.array([[int(v) * N % q for v in row] for row in base[:, first:first + words]], dtype=np.uint64)
    polys = np.zeros((2, N, n), dtype=np.uint64)
    polys[:, :, 0] = 1
    d_rows, d_polys = _dev(torch, _repeat(base, 1, N)), _dev(torch, polys)          # [2][N][words]: term_stride = N
    d_out = _empty(torch, 2, ctx.commitment_words)
    d_status = torch.full((2,), STATUS_SENTINEL, dtype=torch.int32, device="cuda")
    ctx.ring_combine_rows_device(d_rows.data_ptr(), N, d_polys.data_ptr(), 2, d_out.data_ptr(), d_status.data_ptr(), term_stride=N, stream=_stream(torch))
    torch.cuda.synchronize()
    assert d_status.cpu().tolist() == [1, 1]
    assert np.array_equal(_host(d_out), want), (kind, count)


# ---- ring handles under P5 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which", MOD_CASES)
def test_ring_mod(pkg, oracle, opened, which):
    """A ring handle takes its sums in groups of what P = p1 p2 carries: max_terms = ring_mod_capacity(P5, 64) = 524287 >= 3001 for
    dot, the Galois dot and matvec (lsr_ring_mod.hip, lsr_ring_mod_matvec.hip: group_max = min(terms, max_terms); a shared b also
    within bhat_rows = min(4096, 2^21 / n) = 4096), at least as many under a bound (matvec_bounded: ring_mod_capacity_bounded) and for
    the Gram form (min(width, capacity, (2^23 / n - outs) / vectors), lsr_ring_mod_gram.hip).  The fold (lsr_ring_mod_fold.hip) splits
    the 4096 challenge rows among the outputs of a chunk: with two outputs a group would be 2048 terms, so the case folds ONE output of
    width 2, whose group is min(terms, capacity, 4096) = 3001.  Each launch runs once per prime, in the FP64 flavour."""
    import torch
    q, n = P5, DEGREE
    assert mod_model.capacity(q, n) >= N and pkg.ring_mod_capacity(q, n) == mod_model.capacity(q, n)
    assert pkg.ring_mod_capacity_bounded(q, n, MOD_BOUND_X) >= N and pkg.ring_mod_capacity_product(q, n, q // 2, q // 2) >= N
    operands, count, want = _mod_plan(oracle, which)
    _assert_can_tell(count, ("ring_mod", which))
    ring = opened(pkg.RingMod(q, n, device=0))
    assert ring.max_terms >= N and ring.primes == mod_model.primes(n)
    assert ring.prime_context(0).uses_f64 and ring.prime_context(1).uses_f64
    s = _stream(torch)
    status = None
    if which in ("dot", "dot_shared", "galois"):
        g, a0, b0 = operands
        shared = which == "dot_shared"
        d_a, d_b = _dev(torch, _repeat(a0, 1, N)), _dev(torch, _repeat(b0[0], 0, N) if shared else _repeat(b0, 1, N))
        d_out = _empty(torch, 2, n)
        if which == "galois":
            ring.ring_dot_galois_device(d_out.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), 2, N, 2, g, s)
        else:
            ring.dot_device(d_out.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), 2, N, 1 if shared else 2, s)
    elif which == "fold":
        v0, p0 = operands
        d_v, d_p = _dev(torch, _repeat(v0, 0, N)), _dev(torch, _repeat(p0[0], 0, N))          # v [N][2][n], p [1][N][n]
        d_out, status = _empty(torch, 2, n), torch.full((1,), STATUS_SENTINEL, dtype=torch.int32, device="cuda")
        ring.fold_device(d_out.data_ptr(), status.data_ptr(), d_v.data_ptr(), d_p.data_ptr(), 1, N, 0, 2, stream=s)
    elif which in ("matvec", "matvec_bounded"):
        m0, x0 = operands
        rows = m0.shape[0]
        d_m, d_x, d_out = _dev(torch, _repeat(m0, 1, N)), _dev(torch, _repeat(x0, 1, N)), _empty(torch, 2, rows, n)
        mat = opened(ring.matrix_device(d_m.data_ptr(), rows, N, s))
        if which == "matvec":
            mat.matvec_device(d_out.data_ptr(), d_x.data_ptr(), 2, s)
        else:
            status = torch.full((2,), STATUS_SENTINEL, dtype=torch.int32, device="cuda")
            mat.matvec_bounded_device(d_out.data_ptr(), status.data_ptr(), d_x.data_ptr(), 2, bound_x=MOD_BOUND_X, stream=s)
    else:
        a0, b0 = operands
        d_a, d_b = _dev(torch, _repeat(a0[:, None, :], 2, N)), _dev(torch, _repeat(b0[:, None, :], 2, N))      # [2][1][N][n]
        d_out, status = _empty(torch, 2, n), torch.full((2,), STATUS_SENTINEL, dtype=torch.int32, device="cuda")
        ring.gram_device(d_out.data_ptr(), status.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), 2, 1, 1, N, stream=s)
    torch.cuda.synchronize()
    assert status is None or status.cpu().tolist() == [1] * status.numel()
    assert _host(d_out).tolist() == want, (which, count)


# ---- CPU: every plan reaches the count its seed was chosen for ------------------------------------------------------------------------------
def test_every_plan_can_tell_at_four_positions_or_more(oracle):
    """(ring_combine_rows is the one case whose operands, committed rows, exist on the device only: its assert rides with the case.)"""
    counts = {("ring_dot",) + c[:2]: _dot_plan(oracle, *c)[2] for c in DOT_CASES}
    counts["ring_fold"] = _fold_plan(oracle, 7)[2]
    counts.update({("ring_dot_galois",) + c[:2]: _galois_plan(oracle, *c)[3] for c in GALOIS_CASES})
    counts["matvec"], counts["matvec_gadget"] = _matvec_plan(oracle, 8)[2], _gadget_plan(oracle, 9)[2]
    counts.update({("ring_gram",) + c[:3]: _gram_plan(oracle, *c)[2] for c in GRAM_CASES})
    counts.update({("ring_scalar_combine",) + c[:4]: _scalar_plan(oracle, c[0], c[1], c[3], c[4])[3] for c in SCALAR_CASES})
    counts.update({("ring_mod", which): _mod_plan(oracle, which)[1] for which in MOD_CASES})
    print(counts)
    assert _sym2_independent_families(oracle, 35) == 0       # why the sym2 case takes b = a (_gram_plan)
    assert all(count >= WANTED for count in counts.values()), {k: v for k, v in counts.items() if v < WANTED}
