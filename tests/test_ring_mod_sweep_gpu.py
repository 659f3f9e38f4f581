"""GPU suite: every tile log-size LT = 1 .. 12 and both arithmetic flavours (FP64, and the integer kernels a process forces with
lsr_set_arith_mode(1)) of the kernels of a ring handle under an arbitrary modulus (RingMod): the fused mul / dot
(ntt_tile_ring_dot_lift<A, LT, BHAT>), the resident-matrix products M x and M G^-1(x) (ntt_tile_ring_mod_matvec<A, LT, RB, GADGET,
BOTH>) and the bounded Gram matrices.  Each LT is its own instantiation (1, 2 or 3 rounds, a last round of LT % 4 bits with its own
lane mapping, 4096/n vectors per tile), so each is launched here, under two moduli:
  top   the largest q the handle admits at n (44 bits and above p1 at n = 2, 39 bits at n = 4096): capacity 1, so every term and every
        matrix column is a group of its own, reduced with `accumulate`, and the planted products n h^2 and -n h^2 lie within
        n (2 h + 1) of the ends of the CRT range, where ring_mod_reduce_word decides the sign;
  P5    the largest prime = 5 (mod 8) below 2^32: a call is one group.

Every output word is compared exactly with the Python-integer models (ring_mod_model, ring_mod_matvec_model, ring_mod_gram_model),
never with another kernel's, and coefficient n - 1 of all-h by all-h also with n h^2 mod q in closed form.  The references of one
(n, q) are computed once and shared by the two flavours.

Shapes per case: batch = 4096/n + 3 (one full tile and a ragged one of three vectors; 2 at n = 4096, and 3 for mul there, whose two
paired products leave the five edge words no polynomial), 3 terms (under P5 also 33, past
the FP64 re-centring period), rows 5 (a full and a ragged row block in both flavours, row 4 a copy of row 0), cols 3, gadget b = 8
(top) or 11 (P5) at its minimum D with two columns of x, Gram ra = 5, rb = 3, width 2, two families.  Device outputs are one vector
or family longer than the call needs and come back with that tail untouched.

One combination does not exist and is asserted as the refusal: the symmetrised Gram form under `top`, which sums two products per
column where P carries one."""
import functools

import numpy as np
import pytest

import ring_gadget_model as gadget
import ring_mod_gram_model as gram_model
import ring_mod_matvec_model as matvec_model
import ring_mod_model as model

pytestmark = pytest.mark.gpu

P5 = model.prime_5_mod_8_below(1 << 32)
SENTINEL = 0x5A5A5A5A5A5A5A5A
STATUS_SENTINEL = 7
TERMS, LONG_TERMS, ROWS, COLS, XCOLS = 3, 33, 5, 3, 2
RA, RB, WIDTH, FAMILIES = 5, 3, 2, 2
PAIRS = RA * (RA + 1) // 2


def _modulus(logn, name):
    return model.largest_admissible(1 << logn) if name == "top" else P5


def _shape(logn):
    """(vectors per tile, batch, the vectors that hold the planted pairs: the first two, and the first and last of the ragged tile)"""
    per_tile = 4096 >> logn
    if logn == 12:
        return per_tile, 2, [0, 1]
    return per_tile, per_tile + 3, [0, 1, per_tile, per_tile + 2]


def _dots(a, b, q):
    """a [batch][terms][n], b [batch or 1][terms][n] -> [batch][n]"""
    a, b = a.tolist(), b.tolist()
    return np.array([model.negacyclic_dot(a[j], b[j if len(b) > 1 else 0], q) for j in range(len(a))], dtype=np.uint64)


def _matvec_with_copied_row(m, x, q):
    """the model's M x for a matrix whose last row is a copy of row 0: that row's outputs are row 0's"""
    assert np.array_equal(m[-1], m[0])
    y = matvec_model.matvec(m[:-1], x, q)
    return np.concatenate([y, y[:, :1]], axis=1)


@functools.lru_cache(maxsize=None)
def _reference(logn, name):
    """operands and the models' results of one (n, q): computed once, read-only, shared by the two flavours"""
    n, q = 1 << logn, _modulus(logn, name)
    h, hp = q // 2, min(q // 2 + 1, q - 1)
    _, batch, pair_vectors = _shape(logn)
    all_h = {v: h for v in pair_vectors}                                       # against `mixed`: h h, h (h + 1), h h, h (h + 1)
    mixed = {v: (hp if i % 2 else h) for i, v in enumerate(pair_vectors)}
    rng = np.random.default_rng(1000 * logn + (name == "top"))
    r = {"q": q, "n": n}

    singles = max(batch, 3)                                                    # (n = 4096: a third product, for the five edge words)
    a, b = model.planted(rng, q, (singles, n), all_h), model.planted(rng, q, (singles, n), mixed)
    r["mul"] = (a, b, _dots(a[:, None], b[:, None], q), _dots(a[:, None], b[1:2, None], q))

    a, b = model.planted(rng, q, (batch, TERMS, n), all_h), model.planted(rng, q, (batch, TERMS, n), mixed)
    r["dot"] = (a, b, _dots(a, b, q), _dots(a, b[1:2], q))
    if name == "P5":
        few = min(3, batch)
        a, b = model.planted(rng, q, (few, LONG_TERMS, n), {0: h, 1: h}), model.planted(rng, q, (few, LONG_TERMS, n), {0: h, 1: hp})
        r["dot33"] = (a, b, _dots(a, b, q))

    def matrix(cols):
        m = model.planted(rng, q, (ROWS, cols, n), {0: h, 1: hp})              # column 0: row 0 all h, row 1 all h + 1
        m[ROWS - 1] = m[0]
        return m

    m, x = matrix(COLS), model.planted(rng, q, (batch, COLS, n), all_h)
    r["matvec"] = (m, x, _matvec_with_copied_row(m, x, q))

    base_log2 = 8 if name == "top" else 11
    digits = gadget.min_digits(q, base_log2)
    m, x = matrix(XCOLS * digits), model.planted(rng, q, (batch, XCOLS, n), mixed)
    z = matvec_model.decomposed(x, q, base_log2, digits)
    r["gadget"] = (base_log2, digits, m, x, z, _matvec_with_copied_row(m, z, q))

    a = model.planted(rng, q, (FAMILIES, RA, WIDTH, n), {0: h, 1: h})
    b = model.planted(rng, q, (FAMILIES, RB, WIDTH, n), {0: h, 1: hp})
    b5 = model.planted(rng, q, (FAMILIES, RA, WIDTH, n), {0: hp, 1: h})
    la, lb, lb5 = a.tolist(), b.tolist(), b5.tolist()
    g = {"cross": gram_model.gram(la, lb, q), "sym": gram_model.gram(la, None, q)}
    if model.capacity(q, n) >= 2:
        g["sym2"] = gram_model.gram_sym2(la, lb5, q)
    shapes = {"cross": (FAMILIES, RA, RB, n), "sym": (FAMILIES, PAIRS, n), "sym2": (FAMILIES, PAIRS, n)}
    r["gram"] = (a, b, b5, {form: (np.array(words, dtype=np.uint64).reshape(shapes[form]), status) for form, (words, status) in g.items()})

    def freeze(value):
        for item in value.values() if isinstance(value, dict) else value:
            if isinstance(item, np.ndarray):
                item.setflags(write=False)
            elif isinstance(item, (tuple, dict)):
                freeze(item)

    freeze(r)
    return r


def _dev(torch, x):
    return torch.from_numpy(np.array(x, dtype=np.uint64, order="C").view(np.int64)).cuda()          # (a copy: the references are read-only)


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _guarded(torch, *shape):
    """A device output one vector (or family) longer than the call needs, filled with a sentinel"""
    return torch.full((shape[0] + 1,) + tuple(shape[1:]), SENTINEL, dtype=torch.int64, device="cuda")


def _check_guarded(torch, d_out, want, what):
    torch.cuda.synchronize()
    got = _host(d_out)
    assert np.array_equal(got[:-1], want), what
    assert bool((got[-1] == np.uint64(SENTINEL)).all()), (what, "the words behind the output were written")
    return got


@pytest.mark.parametrize("logn", range(1, 13))
@pytest.mark.parametrize("name", ["top", "P5"])
@pytest.mark.parametrize("flavour", ["f64", "u64"])
def test_every_tile_size_flavour_and_modulus_edge(pkg, lib, flavour, name, logn):
    import torch
    n, q = 1 << logn, _modulus(logn, name)
    h, (p1, p2) = q // 2, model.primes(n)
    _, batch, pair_vectors = _shape(logn)
    if name == "top":
        half_p = (p1 * p2 - 1) // 2
        assert model.capacity(q, n) == 1 and model.capacity(q + 1, n) == 0 and half_p - n * h * h < n * (2 * h + 1)
        assert (q > p1) == (logn == 1)                   # n = 2: LiftSource::rebase = p - q wraps, and p1 mod q = p1
    else:
        assert model.capacity(q, n) >= 8191
    ref = _reference(logn, name)
    f64 = flavour == "f64"
    lib.lsr_set_arith_mode(0 if f64 else 1)
    try:
        ring = pkg.RingMod(q, n, device=0)
    finally:
        lib.lsr_set_arith_mode(0)
    where = (flavour, name, n)
    closed = n * h * h % q                               # coefficient n - 1 of all-h by all-h: no wrapped term there
    with ring:
        for i in range(2):
            assert ring.prime_context(i).uses_f64 == f64, where
        assert ring.max_terms == model.capacity(q, n) and ring.primes == (p1, p2)
        stream = _stream(torch)

        # 1. mul: per-product b, one shared b;  2. in place over a
        a, b, want_each, want_shared = ref["mul"]
        singles = a.shape[0]
        d_a, d_b = _dev(torch, a), _dev(torch, b)
        d_c = _guarded(torch, singles, n)
        ring.mul_device(d_c.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), singles, singles, stream=stream)
        got = _check_guarded(torch, d_c, want_each, (where, "mul_device"))
        for v in pair_vectors[0::2]:
            assert int(got[v, n - 1]) == closed, (where, "mul_device, closed form", v)
        d_c = _guarded(torch, singles, n)
        ring.mul_device(d_c.data_ptr(), d_a.data_ptr(), d_b[1].data_ptr(), singles, 1, stream=stream)
        _check_guarded(torch, d_c, want_shared, (where, "mul_device, shared b"))
        d_c = _guarded(torch, singles, n)
        d_c[:singles].copy_(d_a)
        ring.mul_device(d_c.data_ptr(), d_c.data_ptr(), d_b.data_ptr(), singles, singles, stream=stream)
        _check_guarded(torch, d_c, want_each, (where, "mul_device in place over a"))

        # 3. dot: per-output b (BHAT false), one shared b (BHAT true);  4. the host form
        a, b, want_each, want_shared = ref["dot"]
        d_a, d_b = _dev(torch, a), _dev(torch, b)
        d_c = _guarded(torch, batch, n)
        ring.dot_device(d_c.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), batch, TERMS, batch, stream=stream)
        _check_guarded(torch, d_c, want_each, (where, "dot_device"))
        d_c = _guarded(torch, batch, n)
        ring.dot_device(d_c.data_ptr(), d_a.data_ptr(), d_b[1].data_ptr(), batch, TERMS, 1, stream=stream)
        _check_guarded(torch, d_c, want_shared, (where, "dot_device, shared b"))
        assert np.array_equal(ring.dot(a, b), want_each), (where, "dot")
        if "dot33" in ref:
            a, b, want = ref["dot33"]
            d_a, d_b = _dev(torch, a), _dev(torch, b)
            d_c = _guarded(torch, a.shape[0], n)
            ring.dot_device(d_c.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), a.shape[0], LONG_TERMS, a.shape[0], stream=stream)
            _check_guarded(torch, d_c, want, (where, "dot_device, 33 terms"))

        # 5. matvec on a matrix from the host and on one from a device buffer
        m, x, want = ref["matvec"]
        d_x = _dev(torch, x)
        assert int(want[0, 0, n - 1]) == (closed + sum(model.dot_coefficient([m[0, c]], [x[0, c]], q, n - 1) for c in range(1, COLS))) % q
        with ring.matrix(m) as mat:
            assert mat.row_block == (4 if f64 else 2) and (mat.rows, mat.cols) == (ROWS, COLS)
            d_y = _guarded(torch, batch, ROWS, n)
            mat.matvec_device(d_y.data_ptr(), d_x.data_ptr(), batch, stream=stream)
            got = _check_guarded(torch, d_y, want, (where, "matvec_device on matrix"))
            assert np.array_equal(got[:-1, ROWS - 1], got[:-1, 0]), (where, "the copy of row 0 in the ragged row block")
        with ring.matrix_device(_dev(torch, m).data_ptr(), ROWS, COLS, stream=stream) as mat:
            d_y = _guarded(torch, batch, ROWS, n)
            mat.matvec_device(d_y.data_ptr(), d_x.data_ptr(), batch, stream=stream)
            _check_guarded(torch, d_y, want, (where, "matvec_device on matrix_device"))

        # 6. the gadget product, and the plain product on the model's own digits
        base_log2, digits, m, x, z, want = ref["gadget"]
        what = "b = %d, D = %d" % (base_log2, digits)
        assert digits == pkg.ring_gadget_min_digits(q, base_log2) >= 1
        with ring.matrix(m) as mat:
            assert mat.row_block == (4 if f64 else 2)
            d_y = _guarded(torch, batch, ROWS, n)
            mat.matvec_gadget_device(d_y.data_ptr(), _dev(torch, x).data_ptr(), batch, base_log2, digits, stream=stream)
            got = _check_guarded(torch, d_y, want, (where, "matvec_gadget_device", what))
            assert np.array_equal(got[:-1, ROWS - 1], got[:-1, 0]), (where, "gadget: the copy of row 0 in the ragged row block")
            d_y = _guarded(torch, batch, ROWS, n)
            mat.matvec_device(d_y.data_ptr(), _dev(torch, z).data_ptr(), batch, stream=stream)
            _check_guarded(torch, d_y, want, (where, "matvec_device on the model's digits", what))

        # 7. Gram: cross, symmetric, symmetrised
        a, b, b5, want = ref["gram"]
        d_a, d_b, d_b5 = _dev(torch, a), _dev(torch, b), _dev(torch, b5)
        assert int(want["cross"][0][0, 0, 0, n - 1]) == (closed + model.dot_coefficient([a[0, 0, 1]], [b[0, 0, 1]], q, n - 1)) % q

        def gram(form):
            d_g = _guarded(torch, *want[form][0].shape) if form in want else _guarded(torch, FAMILIES, PAIRS, n)
            d_status = torch.full((FAMILIES + 1,), STATUS_SENTINEL, dtype=torch.int32, device="cuda")
            if form == "sym2":
                ring.gram_sym2_device(d_g.data_ptr(), d_status.data_ptr(), d_a.data_ptr(), d_b5.data_ptr(), FAMILIES, RA, WIDTH, stream=stream)
            else:
                ring.gram_device(d_g.data_ptr(), d_status.data_ptr(), d_a.data_ptr(), d_b.data_ptr() if form == "cross" else None, FAMILIES, RA,
                                 RB if form == "cross" else RA, WIDTH, stream=stream)
            _check_guarded(torch, d_g, want[form][0], (where, "gram", form))
            assert want[form][1] == [1] * FAMILIES
            assert d_status.tolist() == [1] * FAMILIES + [STATUS_SENTINEL], (where, "gram status", form)

        gram("cross")
        gram("sym")
        if name == "top":                                # P carries one product, the symmetrised form sums two per column
            assert "sym2" not in want
            with pytest.raises(pkg.CoreError, match="cross form"):
                gram("sym2")
        else:
            gram("sym2")
