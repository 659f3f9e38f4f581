"""GPU suite: the coefficient-wise ring calls on the coefficient context of a ring handle (RingMod.coeff_context,
lsr_ring_mod_coeff_context) under moduli that no NttContext admits — a prime = 5 (mod 8), powers of two, a 41-bit odd
q, Kyber's 3329 at n = 256, an even q that is no power of two, q = 2 and q = 3, and the largest q the handle admits at n = 2 (above
p1) — in both forms (device buffers and host arrays) and both arithmetic flavours (FP64, and the integer kernels a process forces with
lsr_set_arith_mode(1)).  Every output is compared with the Python-integer models of the family (ring_sample_model,
ring_challenge_model, ring_pack_model, ring_gadget_model, ring_galois_model, ring_norm_model, ring_backproject_model,
ring_scalar_model), which take q as a parameter, never with another kernel.

Operands come from ring_mod_model.planted: 0, 1, floor(q/2), floor(q/2) + 1 and q - 1 occur in every array.  The device form takes 64
elements at n <= 256 (at n = 64 a full 4096-word run) and the host form 3 (a ragged run); n = 4096 takes 3 and 2.  Vectors are at
most 4 wide.  Handles are created once per (q, n, flavour) and shared by the module; the references of one (family, q, n) are
computed once and shared by the two flavours.

Where the contract of a call excludes a modulus, the test says so instead of running it: BOUNDED needs 1 <= beta <= (q - 1) / 2 (none
at q = 2), coefficients +-2 need q >= 5, a gadget base B needs B / 2 <= q / 2, CENTRED packing needs a bound of at least 1, and no
|coefficient| can break a bound of 1 at q <= 3."""
import ctypes
import functools

import numpy as np
import pytest

import ring_backproject_model as bmodel
import ring_challenge_model as cmodel
import ring_gadget_model as gmodel
import ring_galois_model as galois
import ring_mod_model as model
import ring_norm_model as nmodel
import ring_pack_model as pmodel
import ring_sample_model as smodel
import ring_scalar_model as scmodel
import test_ring_mod_coeff_abi as abi

pytestmark = pytest.mark.gpu

P5 = 4294967197
TOP2 = model.largest_admissible(2)
CASES = [(64, P5), (64, 1 << 32), (64, (1 << 40) + 15), (256, 3329), (64, 6658), (64, 2), (64, 3), (2, TOP2), (4096, 1 << 32)]
CASE_IDS = ["n%d-q%d" % c for c in CASES]
FLAVOURS = ["f64", "u64"]
UNIFORM, BOUNDED, BALL = 0, 1, 2
CENTRED, RESIDUE = 0, 1
ALL_ONES_64 = 2**64 - 1


def test_the_moduli_are_what_the_suite_says():
    assert P5 == model.prime_5_mod_8_below(1 << 32) and P5 % 8 == 5
    p1, p2 = model.primes(2)
    assert TOP2 > p1 and model.capacity(TOP2, 2) == 1 and model.capacity(TOP2 + 1, 2) == 0
    for n, q in CASES:
        assert model.capacity(q, n) >= 1 and q < 1 << 45


@pytest.fixture(scope="module")
def rings(pkg, lib):
    """{(q, n, flavour): RingMod}, created on first use and closed with the module"""
    made = {}

    def get(q, n, flavour):
        if (q, n, flavour) not in made:
            lib.lsr_set_arith_mode(0 if flavour == "f64" else 1)
            try:
                made[q, n, flavour] = pkg.RingMod(q, n, device=0)
                made[q, n, flavour].coeff_context()
            finally:
                lib.lsr_set_arith_mode(0)
        return made[q, n, flavour]

    yield get
    for ring in made.values():
        ring.close()


@pytest.fixture(params=[(c, f) for f in FLAVOURS for c in CASES], ids=["%s-%s" % (f, i) for f in FLAVOURS for i in CASE_IDS])
def case(request, rings):
    (n, q), flavour = request.param
    ctx = rings(q, n, flavour).coeff_context()
    assert ctx.uses_f64 == (flavour == "f64") and (ctx.q, ctx.n) == (q, n)
    return ctx, q, n


def _oracle():
    import oracle_binding
    return oracle_binding.load()


def _counts(n):
    return (64, 3) if n <= 256 else (3, 2)


def _dev(torch, x, dtype=np.uint64):
    return torch.from_numpy(np.array(x, dtype=dtype, order="C").view(np.int64 if dtype == np.uint64 else dtype)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _empty(torch, *shape):
    return torch.full(shape, 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")


def _status(torch, count):
    return torch.full((count,), 7, dtype=torch.int32, device="cuda")


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _keys(seed, groups):
    return [smodel.key_from_seed(seed + i) for i in range(groups)]


def _karr(keys):
    return np.array(keys, dtype=np.uint64).reshape(-1, 4)


def _rng(n, q, salt):
    return np.random.default_rng([n, q % (1 << 32), q >> 32, salt])


def _with_bad_word(x, q, vector):
    """a copy of x whose vector `vector` holds one word >= q (q itself)"""
    y = np.array(x, dtype=np.uint64)
    y[vector].reshape(-1)[-1] = q
    return y


def _ints128(pairs):
    return [int(lo) | (int(hi) << 64) for lo, hi in pairs.tolist()]


# ---- sample --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sample_ref(n, q):
    dev_count, host_count = _counts(n)
    kinds = [(UNIFORM, 0), (BALL, min(n, 31))] + ([(BOUNDED, min((q - 1) // 2, 1000))] if q >= 3 else [])
    keys, ref = _keys(100 + n, 2), {}
    for kind, param in kinds:
        for count in (dev_count, host_count):
            ref[kind, param, count] = smodel.sample(_oracle(), q, n, count, kind, param, keys, -(-count // 2), 16, 5)[0]
    return keys, ref


def test_sample(pkg, case):
    import torch
    ctx, q, n = case
    dev_count, host_count = _counts(n)
    keys, ref = _sample_ref(n, q)
    assert {k for k, _, _ in ref} == ({UNIFORM, BALL, BOUNDED} if q >= 3 else {UNIFORM, BALL})
    d_keys = _dev(torch, _karr(keys))
    for (kind, param, count), want in ref.items():
        assert int(want.max()) < q
        if count == dev_count:
            d_out = _empty(torch, count, n)
            ctx.ring_sample_device(d_out.data_ptr(), count, kind, param, d_keys.data_ptr(), -(-count // 2), 16, 5, stream=_stream(torch))
            torch.cuda.synchronize()
            assert np.array_equal(_host(d_out), want), (kind, param, "device")
        if count == host_count:
            assert np.array_equal(ctx.ring_sample(count, kind, param, _karr(keys), -(-count // 2), 16, 5), want), (kind, param, "host")
    if q == 2:
        with pytest.raises(pkg.CoreError, match="BOUNDED takes"):
            ctx.ring_sample(1, BOUNDED, 1, _karr(keys))


# ---- challenge and operator norm -------------------------------------------------------------------------------------------------------------
def _challenge_shapes(n, q):
    k1, k2 = (31, 10) if n >= 64 else (1, 1)
    if q < 5:
        k1, k2 = k1 + k2 - 10 if n >= 64 else 1, 0
    return [(k1, k2, 15), (k1, k2, 0)] if n == 64 else [(k1, k2, 0)]


@functools.lru_cache(maxsize=None)
def _challenge_ref(n, q):
    dev_count, host_count = (16, 3) if n <= 256 else (3, 2)
    keys, ref = _keys(200 + n, 2), {}
    for k1, k2, bound in _challenge_shapes(n, q):
        for count in (dev_count, host_count):
            out, tries, _ = cmodel.challenge(_oracle(), q, n, count, k1, k2, bound, 256, keys, -(-count // 2), 16, 9)
            ref[k1, k2, bound, count] = (out, tries)
    return keys, ref, dev_count, host_count


def test_challenge(case):
    import torch
    ctx, q, n = case
    keys, ref, dev_count, host_count = _challenge_ref(n, q)
    d_keys = _dev(torch, _karr(keys))
    for (k1, k2, bound, count), (want, want_tries) in ref.items():
        assert bound == 0 or int(want_tries.min()) >= 1                     # the model found every element within max_tries
        if count == dev_count:
            d_out, d_tries = _empty(torch, count, n), _status(torch, count)
            ctx.ring_challenge_device(d_out.data_ptr(), d_tries.data_ptr(), count, k1, k2, bound, d_keys.data_ptr(), -(-count // 2), max_tries=256,
                                      domain=16, index_base=9, stream=_stream(torch))
            torch.cuda.synchronize()
            assert np.array_equal(_host(d_out), want) and d_tries.cpu().tolist() == want_tries.tolist(), (k1, k2, bound, "device")
        if count == host_count:
            out, tries = ctx.ring_challenge(count, k1, k2, bound, _karr(keys), -(-count // 2), 256, 16, 9)
            assert np.array_equal(out, want) and tries.tolist() == want_tries.tolist(), (k1, k2, bound, "host")


@functools.lru_cache(maxsize=None)
def _opnorm_ref(n, q):
    keys, ref, dev_count, _ = _challenge_ref(n, q)
    short = next(iter(ref.values()))[0][:3]                                  # three challenges: short elements
    x = np.concatenate([short, model.planted(_rng(n, q, 3), q, (3, n)), _with_bad_word(short[:1], q, 0)])
    return x, [cmodel.opnorm(row.tolist(), q) for row in x]


def test_opnorm(case):
    import torch
    ctx, q, n = case
    x, want = _opnorm_ref(n, q)
    assert want[-1] == cmodel.ALL_ONES and want[0] != cmodel.ALL_ONES
    ctx.ring_opnorm_prepare()
    d_out = _empty(torch, len(x), 2)
    d_x_in = _dev(torch, x)      # (kept alive across the call)
    ctx.ring_opnorm_device(d_x_in.data_ptr(), len(x), d_out.data_ptr(), stream=_stream(torch))
    torch.cuda.synchronize()
    assert _ints128(_host(d_out)) == want, "device"
    assert list(ctx.ring_opnorm(x)) == want, "host"


# ---- pack and unpack ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pack_ref(n, q):
    dev_count, _ = _counts(n)
    rng, ref = _rng(n, q, 4), {}
    for mode in (CENTRED, RESIDUE):
        bound = min((q - 1) // 2, 1000) if mode == CENTRED else min(q - 1, 1000)
        bits = pmodel.min_bits(q, mode, bound)
        if bits == 0:
            assert q == 2 and mode == CENTRED
            continue
        x = np.array([pmodel.in_range_element(rng, n, q, bits, mode) for _ in range(dev_count)], dtype=np.uint64)
        x[1, n // 2] = q // 2                      # out of range wherever the range is narrower than the ring
        x[2, n - 1] = q                            # a word >= q
        words, status = pmodel.pack_array(x, q, bits, mode)
        packed = np.array(words[:dev_count], dtype=np.uint64)
        packed[2] = ALL_ONES_64                    # fields of all ones, and padding bits where n bits is no multiple of 64
        back, back_status = pmodel.unpack_array(packed, n, q, bits, mode)
        ref[mode] = (bound, bits, x, words, status, packed, back, back_status)
    return ref


def test_pack_and_unpack(pkg, case):
    import torch
    ctx, q, n = case
    ref = _pack_ref(n, q)
    assert (CENTRED in ref) == (q > 2) and RESIDUE in ref
    for mode, (bound, bits, x, words, status, packed, back, back_status) in ref.items():
        assert pkg.ring_pack_min_bits(q, mode, bound) == bits and pkg.ring_pack_words(n, bits) == words.shape[1]
        count = len(x)
        assert status[2] == -1 and status[0] == 1 and (status[1] == 0) == (not pmodel.field_range(mode, bits)[0] <= (
            pmodel.centre(q // 2, q) if mode == CENTRED else q // 2) <= pmodel.field_range(mode, bits)[1])
        assert back_status[0] == 1 and np.array_equal(back[0], x[0])
        d_out, d_status = _empty(torch, count, words.shape[1]), _status(torch, count)
        d_x_in = _dev(torch, x)      # (kept alive across the call)
        ctx.ring_pack_device(d_out.data_ptr(), d_status.data_ptr(), d_x_in.data_ptr(), count, bits, mode, stream=_stream(torch))
        torch.cuda.synchronize()
        assert np.array_equal(_host(d_out), words) and d_status.cpu().tolist() == status.tolist(), (mode, "pack, device")
        got, got_status = ctx.ring_pack(x[:3], bits, mode)
        assert np.array_equal(got, words[:3]) and got_status.tolist() == status[:3].tolist(), (mode, "pack, host")
        d_out, d_status = _empty(torch, count, n), _status(torch, count)
        d_packed_in = _dev(torch, packed)      # (kept alive across the call)
        ctx.ring_unpack_device(d_out.data_ptr(), d_status.data_ptr(), d_packed_in.data_ptr(), count, bits, mode, stream=_stream(torch))
        torch.cuda.synchronize()
        assert np.array_equal(_host(d_out), back) and d_status.cpu().tolist() == back_status.tolist(), (mode, "unpack, device")
        got, got_status = ctx.ring_unpack(packed[:3], bits, mode)
        assert np.array_equal(got, back[:3]) and got_status.tolist() == back_status[:3].tolist(), (mode, "unpack, host")


# ---- gadget digits and the l-infinity norm ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gadget_ref(n, q):
    dev_count, _ = _counts(n)
    rng = _rng(n, q, 5)
    x = model.planted(rng, q, (dev_count, n))
    ref = {}
    for b in (8, 11):
        digits = gmodel.min_digits(q, b)
        z = gmodel.decompose(x, q, b, digits) if digits else None
        any_digits = digits or 2
        r = rng.integers(0, q, size=(dev_count, any_digits, n), dtype=np.uint64)      # recompose takes any canonical residues
        ref[b] = (digits, z, r, gmodel.recompose(r, q, b))
    bad = _with_bad_word(x, q, 1)
    return x, ref, bad, gmodel.linf(bad, q)


def test_decompose_recompose_linf(pkg, case):
    import torch
    ctx, q, n = case
    x, ref, bad, want_linf = _gadget_ref(n, q)
    count = len(x)
    d_x = _dev(torch, x)
    for b, (digits, z, r, want_r) in ref.items():
        assert pkg.ring_gadget_min_digits(q, b) == digits and (digits == 0) == ((1 << (b - 1)) > q // 2)
        if digits:
            assert np.array_equal(gmodel.recompose(z, q, b), x)
            d_z = _empty(torch, count, digits, n)
            ctx.ring_decompose_device(d_z.data_ptr(), d_x.data_ptr(), count, b, digits, stream=_stream(torch))
            torch.cuda.synchronize()
            assert np.array_equal(_host(d_z), z), (b, "decompose, device")
            assert np.array_equal(ctx.ring_decompose(x[:3], b, digits), z[:3]), (b, "decompose, host")
        d_out = _empty(torch, count, n)
        d_r_in = _dev(torch, r)      # (kept alive across the call)
        ctx.ring_recompose_device(d_out.data_ptr(), d_r_in.data_ptr(), count, b, r.shape[1], stream=_stream(torch))
        torch.cuda.synchronize()
        assert np.array_equal(_host(d_out), want_r), (b, "recompose, device")
        assert np.array_equal(ctx.ring_recompose(r[:3], b), want_r[:3]), (b, "recompose, host")
    assert int(want_linf[1]) == ALL_ONES_64 and (n < 8 or int(want_linf[0]) == q // 2)
    d_out = _empty(torch, count)
    d_bad_in = _dev(torch, bad)      # (kept alive across the call)
    ctx.ring_linf_device(d_bad_in.data_ptr(), count, d_out.data_ptr(), stream=_stream(torch))
    torch.cuda.synchronize()
    assert np.array_equal(_host(d_out), want_linf), "linf, device"
    assert np.array_equal(ctx.ring_linf(bad[:3]), want_linf[:3]), "linf, host"


# ---- automorphisms ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _automorphism_ref(n, q):
    dev_count, _ = _counts(n)
    x = model.planted(_rng(n, q, 6), q, (dev_count, n))
    return x, {g: galois.automorphism_np(x, g, q, -1) for g in sorted({1, 3, 5, 2 * n - 1}) if g < 2 * n}


def test_automorphism(case):
    import torch
    ctx, q, n = case
    x, want = _automorphism_ref(n, q)
    assert want[1].tolist() == x.tolist() and galois.automorphism(x[0].tolist(), 2 * n - 1, q, -1) == want[2 * n - 1][0].tolist()
    d_x = _dev(torch, x)
    for g, w in want.items():
        d_out = _empty(torch, len(x), n)
        ctx.ring_automorphism_device(d_out.data_ptr(), d_x.data_ptr(), len(x), g, stream=_stream(torch))
        torch.cuda.synchronize()
        assert np.array_equal(_host(d_out), w), (g, "device")
        assert np.array_equal(ctx.ring_automorphism(x[:3], g), w[:3]), (g, "host")


# ---- l2 norms and projections ---------------------------------------------------------------------------------------------------------------
def _vectors(n, q, salt, width):
    dev_count, _ = _counts(n)
    count = max(3, dev_count // width)
    return model.planted(_rng(n, q, salt), q, (count, width, n))


@functools.lru_cache(maxsize=None)
def _l2sq_ref(n, q):
    x = _with_bad_word(_vectors(n, q, 7, 4), q, 2)
    return x, nmodel.l2sq(q, x)


def test_l2sq(case):
    import torch
    ctx, q, n = case
    x, want = _l2sq_ref(n, q)
    assert want[2] == nmodel.SATURATED and want[0] < nmodel.SATURATED
    d_out = _empty(torch, len(x), 2)
    d_x_in = _dev(torch, x)      # (kept alive across the call)
    ctx.ring_l2sq_device(d_x_in.data_ptr(), len(x), 4, d_out.data_ptr(), stream=_stream(torch))
    torch.cuda.synchronize()
    assert _ints128(_host(d_out)) == want, "device"
    assert list(ctx.ring_l2sq(x[:3])) == want[:3], "host"


@functools.lru_cache(maxsize=None)
def _project_ref(n, q):
    width = 3
    x = _with_bad_word(_vectors(n, q, 8, width), q, 1)
    count = len(x)
    keys, components = _keys(300 + n, 2), -(-count // 2)
    bounds = [q // 2] + ([max(1, q // 4)] if q > 3 else [])                 # kept (but for the word >= q); broken by the planted edges
    return x, keys, components, {b: nmodel.project(_oracle(), q, x, b, keys, components, 17, 11) for b in bounds}


def test_project(case):
    import torch
    ctx, q, n = case
    x, keys, components, want = _project_ref(n, q)
    count = len(x)
    kept = want[q // 2][1].tolist()
    assert kept[1] == -1 and all(s == 1 for i, s in enumerate(kept) if i != 1)
    if q > 3:
        assert 0 in want[max(1, q // 4)][1].tolist()
    d_x, d_keys = _dev(torch, x), _dev(torch, _karr(keys))
    for bound, (p, status) in want.items():
        d_out, d_status = torch.full((count, 256), -7, dtype=torch.int64, device="cuda"), _status(torch, count)
        ctx.ring_project_device(d_out.data_ptr(), d_status.data_ptr(), d_x.data_ptr(), count, 3, bound, d_keys.data_ptr(), components, 17, 11,
                                stream=_stream(torch))
        torch.cuda.synchronize()
        assert np.array_equal(d_out.cpu().numpy(), p) and d_status.cpu().tolist() == status.tolist(), (bound, "device")
        got, got_status = ctx.ring_project(x, bound, _karr(keys), components, 17, 11)
        assert np.array_equal(got, p) and got_status.tolist() == status.tolist(), (bound, "host")


@functools.lru_cache(maxsize=None)
def _project_matrix_ref(n, q):
    key, width = smodel.key_from_seed(400 + n), 2 if n > 256 else 4
    return key, width, {(first, rows): nmodel.project_matrix(_oracle(), q, n, width, key, first, rows, 17, 13) for first, rows in ((0, 256), (37, 5))}


def test_project_matrix(case):
    import torch
    ctx, q, n = case
    key, width, want = _project_matrix_ref(n, q)
    d_key = _dev(torch, _karr([key]))
    for (first, rows), w in want.items():
        assert set(np.unique(w).tolist()) <= {0, 1, q - 1}
        d_out = _empty(torch, rows, width, n)
        ctx.ring_project_matrix_device(d_out.data_ptr(), first, rows, width, d_key.data_ptr(), 17, 13, stream=_stream(torch))
        torch.cuda.synchronize()
        assert np.array_equal(_host(d_out), w), (first, rows, "device")
        assert np.array_equal(ctx.ring_project_matrix(_karr([key]), width, first, rows, 17, 13), w), (first, rows, "host")


@functools.lru_cache(maxsize=None)
def _adjoint_ref(n, q):
    count, width, components = 3, 2, 2
    keys, rng, ref = _keys(500 + n, 2), _rng(n, q, 9), {}
    for sets in (1, 3):
        weights = model.planted(rng, q, (2, sets, 256))
        for conjugate in (False, True):
            ref[sets, conjugate] = (weights, bmodel.back_project(_oracle(), q, n, width, weights.tolist(), count, keys, components, 17, 15, conjugate))
    return count, width, components, keys, ref


def test_project_adjoint(case):
    import torch
    ctx, q, n = case
    count, width, components, keys, ref = _adjoint_ref(n, q)
    d_keys = _dev(torch, _karr(keys))
    for (sets, conjugate), (weights, (want, status)) in ref.items():
        assert status.tolist() == [1] * count
        d_out, d_status = _empty(torch, count, sets, width, n), _status(torch, count)
        d_weights_in = _dev(torch, weights)      # (kept alive across the call)
        ctx.ring_project_adjoint_device(d_out.data_ptr(), d_status.data_ptr(), d_weights_in.data_ptr(), count, sets, width, conjugate,
                                        d_keys.data_ptr(), components, 17, 15, stream=_stream(torch))
        torch.cuda.synchronize()
        assert np.array_equal(_host(d_out), want) and d_status.cpu().tolist() == status.tolist(), (sets, conjugate, "device")
        got, got_status = ctx.ring_project_adjoint(weights, width, count, _karr(keys), components, conjugate, 17, 15)
        assert np.array_equal(got, want) and got_status.tolist() == status.tolist(), (sets, conjugate, "host")


# ---- scalar aggregation ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scalar_ref(n, q):
    count, width, terms, components = 3, 2, 5, 2
    rng, ref = _rng(n, q, 10), {}
    v = model.planted(rng, q, (count * terms, width, n))
    for sets in ((1, 3, 16) if n <= 256 else (3,)):
        weights = model.planted(rng, q, (2, sets, terms))
        addend = model.planted(rng, q, (count, sets, width, n))
        for stride in (0, terms):
            ref[sets, stride] = (weights, addend, scmodel.scalar_combine(q, n, width, v, weights, addend, count, stride, components))
    return count, width, terms, components, v, ref


def test_scalar_combine(case):
    import torch
    ctx, q, n = case
    count, width, terms, components, v, ref = _scalar_ref(n, q)
    d_v = _dev(torch, v)
    for (sets, stride), (weights, addend, (want, status)) in ref.items():
        assert status.tolist() == [1] * count
        d_out, d_status = _dev(torch, addend), _status(torch, count)        # the addend in place
        d_weights_in = _dev(torch, weights)      # (kept alive across the call)
        ctx.ring_scalar_combine_device(d_out.data_ptr(), d_status.data_ptr(), d_v.data_ptr(), d_weights_in.data_ptr(), d_out.data_ptr(), count,
                                       sets, terms, stride, width, components, stream=_stream(torch))
        torch.cuda.synchronize()
        assert np.array_equal(_host(d_out), want) and d_status.cpu().tolist() == status.tolist(), (sets, stride, "device")
        got, got_status = ctx.ring_scalar_combine(v, weights, count, stride, components, addend)
        assert np.array_equal(got, want) and got_status.tolist() == status.tolist(), (sets, stride, "host")


# ---- the word-by-word product --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pointwise_ref(n, q):
    dev_count, _ = _counts(n)
    rng = _rng(n, q, 11)
    a, b = model.planted(rng, q, (dev_count, n)), model.planted(rng, q, (dev_count, n))
    b[0] = a[0]                                                            # the edge words against themselves
    want = np.array([[int(x) * int(y) % q for x, y in zip(ra, rb)] for ra, rb in zip(a.tolist(), b.tolist())], dtype=np.uint64)
    return a, b, want


def test_pointwise_product(pkg, lib, case):
    import torch
    ctx, q, n = case
    a, b, want = _pointwise_ref(n, q)
    count = len(a)
    d_out = _empty(torch, count, n)
    d_a_in, d_b_in = _dev(torch, a), _dev(torch, b)      # (kept alive across the call)
    ctx.mul_pointwise_device(d_out.data_ptr(), d_a_in.data_ptr(), d_b_in.data_ptr(), count * n, stream=_stream(torch))
    torch.cuda.synchronize()
    assert np.array_equal(_host(d_out), want), "lsr_ntt_mul_pointwise_device"
    assert np.array_equal(ctx.mul_pointwise(a[0], b[0]), want[0]), "ntt_mul_pointwise"
    out = np.zeros((3, n), dtype=np.uint64)
    a3, b3 = np.ascontiguousarray(a[:3]), np.ascontiguousarray(b[:3])
    assert lib.ntt_mul_pointwise_batch(ctx.handle, out.ctypes.data, a3.ctypes.data, b3.ctypes.data, 3) == 0
    assert np.array_equal(out, want[:3]), "ntt_mul_pointwise_batch"


# ---- accessors and refusals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_accessors(pkg, lib, rings, flavour):
    ring = rings(P5, 64, flavour)
    ctx = ring.coeff_context()
    assert ctx is ring.coeff_context() and ctx.handle and ctx.handle not in (ring.prime_context(0).handle, ring.prime_context(1).handle)
    assert lib.lsr_ntt_context_device(ctx.handle) == 0 and ctx.root == 0 and ctx.uses_f64 == (flavour == "f64") and ctx.handoff_bytes == 8
    assert lib.lsr_ntt_context_is_cyclic(ctx.handle) == 0
    lib.ntt_context_free(ctx.handle)                                       # does nothing: the handle owns it
    x = model.planted(_rng(64, P5, 12), P5, (3, 64))
    assert np.array_equal(ctx.ring_automorphism(x, 1), x)
    with pkg.RingMod(1 << 32, 8192, device=0) as big:                      # above 4096: no packed hand-off either
        assert big.coeff_context().handoff_bytes == 8 and big.coeff_context().uses_f64


def test_a_closed_ring_lets_its_coefficient_context_go(pkg):
    ring = pkg.RingMod(3329, 256, device=0)
    ctx = ring.coeff_context()
    ring.close()
    assert ctx.handle is None


@pytest.mark.parametrize("name", sorted(abi.REFUSED))
def test_refused_on_the_coefficient_context(pkg, lib, rings, name):
    """the call built from SIGNATURES with the coefficient context and zeros elsewhere: refused before any buffer is looked at.  (A
    sharded call takes its contexts as an array: the array holds the context and `shards` says one.)"""
    ctx = rings(P5, 64, "f64").coeff_context()
    result, arguments = pkg._abi.SIGNATURES[name]
    args = [ctx.handle] + [0 if a is not ctypes.c_void_p else None for a in arguments[1:]]
    if name.endswith("_sharded"):
        array = (ctypes.c_void_p * 1)(ctx.handle)
        args[0], args[1] = ctypes.addressof(array), 1
    lib.lsr_ring_mod_max_terms(None)                                       # (any call: the message below is this call's own)
    got = getattr(lib, name)(*args)
    assert got == (-1 if result is ctypes.c_int else 0 if result is ctypes.c_size_t else None), name
    msg = pkg._abi.last_error()
    assert msg.startswith(name + ":") and "coefficient context" in msg, msg
    instead = abi.REFUSED[name]
    assert (": use " not in msg) if instead is None else ("use " + instead + " on the handle" in msg), msg


def test_members_that_transform_raise_on_it(pkg, rings):
    ctx = rings(P5, 64, "f64").coeff_context()
    x = np.zeros((2, 64), dtype=np.uint64)
    with pytest.raises(pkg.CoreError, match="coefficient context"):
        ctx.ring_mul(x, x)
    with pytest.raises(pkg.CoreError, match="lsr_ring_mod_dot_galois_batch"):
        ctx.ring_dot_galois(x, x, 3)
    with pytest.raises(pkg.CoreError, match="coefficient context"):
        ctx.forward_batch(x)


# ---- the chain the feature exists for ---------------------------------------------------------------------------------------------------------
def test_projection_equals_the_constant_term_of_the_twisted_inner_product(pkg, oracle, rings):
    """Device-resident under q = 4294967197, n = 64: a witness s sampled BOUNDED, p = Pi s by ring_project, the rows pi_r by
    ring_project_matrix, and c_r = sum_w sigma_{2n-1}(pi_{r,w}) s_w by RingMod.ring_dot_galois_device: coefficient 0 of c_r is p_r mod q."""
    import torch
    q, n, width, beta, rows = P5, 64, 4, 1000, 4
    ring = rings(q, n, "f64")
    ctx = ring.coeff_context()
    key = smodel.key_from_seed(77)
    d_key, stream = _dev(torch, _karr([key])), _stream(torch)
    d_s = _empty(torch, width, n)
    ctx.ring_sample_device(d_s.data_ptr(), width, BOUNDED, beta, d_key.data_ptr(), width, 16, 0, stream=stream)
    d_p, d_status = torch.zeros((1, 256), dtype=torch.int64, device="cuda"), _status(torch, 1)
    ctx.ring_project_device(d_p.data_ptr(), d_status.data_ptr(), d_s.data_ptr(), 1, width, beta, d_key.data_ptr(), 1, 17, 0, stream=stream)
    d_rows = _empty(torch, rows, width, n)
    ctx.ring_project_matrix_device(d_rows.data_ptr(), 0, rows, width, d_key.data_ptr(), 17, 0, stream=stream)
    d_c = _empty(torch, rows, n)
    ring.ring_dot_galois_device(d_c.data_ptr(), d_rows.data_ptr(), d_s.data_ptr(), rows, width, 1, 2 * n - 1, stream=stream)
    torch.cuda.synchronize()
    s, p, c = _host(d_s), d_p.cpu().numpy()[0], _host(d_c)
    assert d_status.cpu().tolist() == [1]
    assert np.array_equal(s, smodel.sample(oracle, q, n, width, BOUNDED, beta, [key], width, 16, 0)[0])
    want = nmodel.project_ints(oracle, q, s.reshape(-1).tolist(), key, 17, 0)
    assert p.tolist() == want
    for r in range(rows):
        assert int(c[r, 0]) == want[r] % q, r
