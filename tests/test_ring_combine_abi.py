"""CPU suite: the ABI surface of the ring-element linear combination of commitment rows (lsr_lwe_ring_combine_rows_device,
lsr_lwe_ring_combine_batch_flat, lsr_lwe_combine_max_weight), the refusals a host without a device can reach, and the self-checks of the
model the GPU tests compare the library with (ring_combine_model.py).  No device work."""
import ctypes
import os
import re

import numpy as np

import combine_model
import ring_combine_model as model
import rns_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLARATIONS = [
    "#define LSR_RING_COMBINE_MAX_TERMS 65536 ",
    "int lsr_lwe_ring_combine_rows_device(const LweContext* ctx, const uint64_t* d_rows, size_t terms, size_t term_stride, const uint64_t* d_polys, "
    "size_t outputs, uint64_t* d_out_rows, int* d_status, void* stream) LSR_NOEXCEPT;",
    "int lsr_lwe_ring_combine_batch_flat(const LweContext* ctx, const uint64_t* rows, size_t terms, size_t term_stride, const uint64_t* polys, "
    "size_t outputs, uint64_t* out_rows, int* status) LSR_NOEXCEPT;",
    "uint64_t lsr_lwe_combine_max_weight(const LweContext* ctx) LSR_NOEXCEPT;",
]
NAMES = ("lsr_lwe_ring_combine_rows_device", "lsr_lwe_ring_combine_batch_flat", "lsr_lwe_combine_max_weight")


def _batch_h():
    text = open(os.path.join(ROOT, "include", "lambda_snark", "batch.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"\s+", " ", text)


def test_symbols_are_declared_exported_and_bound(pkg, lib):
    h = _batch_h()
    for line in DECLARATIONS:
        assert line in h, line
    vp, size, cint = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    sig = pkg._abi.SIGNATURES
    assert sig["lsr_lwe_ring_combine_rows_device"] == (cint, [vp, vp, size, size, vp, size, vp, vp, vp])
    assert sig["lsr_lwe_ring_combine_batch_flat"] == (cint, [vp, vp, size, size, vp, size, vp, vp])
    assert sig["lsr_lwe_combine_max_weight"] == (ctypes.c_uint64, [vp])
    for name in NAMES:
        fn = getattr(lib, name)
        assert fn.restype is sig[name][0] and list(fn.argtypes) == sig[name][1]
    assert pkg._abi.RING_COMBINE_MAX_TERMS == 65536
    assert callable(pkg.LweContext.ring_combine_rows_device) and callable(pkg.LweContext.ring_combine_rows)
    assert isinstance(pkg.LweContext.combine_max_weight, property)


def test_refusals_without_a_device(lib):
    """Without a device no context can exist, so the NULL context is the one argument error a host without a GPU can reach; the refusals
    that need a live context are in the GPU suite."""
    buf = np.zeros(8, dtype=np.uint64)
    out = np.zeros(8, dtype=np.uint64)
    status = np.full(1, 7, dtype=np.int32)
    calls = {
        b"lsr_lwe_ring_combine_rows_device": lambda outputs: lib.lsr_lwe_ring_combine_rows_device(None, buf.ctypes.data, 1, 0, buf.ctypes.data, outputs,
                                                                                                  out.ctypes.data, status.ctypes.data, None),
        b"lsr_lwe_ring_combine_batch_flat": lambda outputs: lib.lsr_lwe_ring_combine_batch_flat(None, buf.ctypes.data, 1, 0, buf.ctypes.data, outputs,
                                                                                                out.ctypes.data, status.ctypes.data),
    }
    for name, call in calls.items():
        for outputs in (1, 0):                    # outputs == 0 does not rescue a NULL context
            assert not lib.lsr_lwe_context_create_rns(None, 3, -1) and b"NULL params" in lib.lsr_last_error()      # another text in between
            assert call(outputs) == -1
            assert name in lib.lsr_last_error() and b"NULL context" in lib.lsr_last_error(), lib.lsr_last_error()
    assert status[0] == 7 and not out.any()       # nothing was written
    assert lib.lsr_lwe_combine_max_weight(None) == 0


def _rows(rng, terms, n, k, moduli, header):
    head, blocks = model.layout(n, k, moduli)
    rows = np.zeros((terms, head + len(moduli) * (k + 1) * n), dtype=np.uint64)
    rows[:, :head] = np.array(header, dtype=np.uint64)
    for first, words, q in blocks:
        rows[:, first:first + words] = rng.integers(0, q, size=(terms, words), dtype=np.uint64)
    return rows


def test_constant_polynomials_reproduce_the_scalar_model():
    rng = np.random.default_rng(3)
    n, k = 64, 2
    t = rns_model.plain_modulus(4096)
    for moduli in ((17592169062401,), rns_model.rns_moduli(4096), ((1 << 60) - 93,)):
        header = model.rns_header(n, k, t, moduli) if len(moduli) == 2 else [8 * (4 + (k + 1) * n), 1, n | (k << 32), moduli[0], t]
        rows = _rows(rng, 5, n, k, moduli, header)
        coeffs = np.array([0, 1, t - 1, t // 2, t // 2 + 1], dtype=np.uint64) + np.array([0, t, 3 * t, 0, t], dtype=np.uint64)
        polys = np.zeros((5, n), dtype=np.uint64)
        polys[:, 0] = coeffs
        polys[2, 5] = t                            # 0 mod t in a higher coefficient: still a constant
        head, blocks = model.layout(n, k, moduli)
        want = combine_model.combine_rows(rows, coeffs, t, head, blocks)
        assert model.combine_row(rows, polys, t, n, k, moduli).tolist() == want
        assert model.weight(polys, t) == combine_model.weight(coeffs, t) == 1 + 1 + t // 2 + t // 2


def test_multiplying_by_x_to_the_n_negates_the_row():
    rng = np.random.default_rng(4)
    n, k, q, t = 128, 1, 17592169062401, rns_model.plain_modulus(4096)
    rows = _rows(rng, 1, n, k, (q,), [8 * (4 + (k + 1) * n), 1, n | (k << 32), q, t])
    x_a, x_b = np.zeros((1, n), dtype=np.uint64), np.zeros((1, n), dtype=np.uint64)
    x_a[0, 37], x_b[0, n - 37] = 1, 1
    once = model.combine_row(rows, x_a, t, n, k, (q,))
    twice = model.combine_row(once[None, :], x_b, t, n, k, (q,))
    head = 5
    assert np.array_equal(twice[:head], rows[0, :head])
    assert twice[head:].tolist() == [(q - int(w)) % q for w in rows[0, head:]]
    # and the centred rule: t - 1 acts as -1, so X^37 with coefficient t - 1 negates `once`
    x_a[0, 37] = t - 1
    assert model.combine_row(rows, x_a, t, n, k, (q,))[head:].tolist() == [(q - int(w)) % q for w in once[head:]]


def test_sparse_and_dense_forms_agree(oracle):
    rng = np.random.default_rng(5)
    n, k = 256, 1
    t = rns_model.plain_modulus(4096)
    for moduli in ((17592169062401,), rns_model.rns_moduli(4096)):
        header = model.rns_header(n, k, t, moduli) if len(moduli) == 2 else [8 * (4 + (k + 1) * n), 1, n | (k << 32), moduli[0], t]
        rows = _rows(rng, 3, n, k, moduli, header)
        polys = np.zeros((3, n), dtype=np.uint64)
        for i in range(3):
            taps = rng.choice(n, size=6, replace=False)
            polys[i, taps] = np.array([1, t - 1, t // 2, t // 2 + 1, t + 5, 2**64 - 1], dtype=np.uint64)
        sparse = model.combine_row(rows, polys, t, n, k, moduli)
        dense = model.combine_row(rows, polys, t, n, k, moduli, oracle=oracle)
        assert np.array_equal(sparse, dense)
        # a dense polynomial through both forms as well
        full = rng.integers(0, 2**63, size=(3, n), dtype=np.uint64)
        assert np.array_equal(model.combine_row(rows, full, t, n, k, moduli), model.combine_row(rows, full, t, n, k, moduli, oracle=oracle))


def test_schoolbook_by_hand_and_against_the_sparse_form():
    q, t = 17592169062401, rns_model.plain_modulus(4096)
    a, p = np.array([[3, q - 5]], dtype=np.uint64), np.array([[2, -7]], dtype=np.int64)
    # (2 - 7X)(3 + (q - 5)X) mod X^2 + 1 = 6 + 7(q - 5) + (2(q - 5) - 21) X
    assert model.dot_schoolbook(a, p, q).tolist() == [(6 + 7 * (q - 5)) % q, (2 * (q - 5) - 21) % q]
    rng = np.random.default_rng(6)
    for n in (2, 4, 16, 64):
        for modulus in (q, rns_model.rns_moduli(n)[1], (1 << 60) - 93):
            residues = rng.integers(0, modulus, size=(3, n), dtype=np.uint64)
            residues[0, 0], residues[2, n - 1] = modulus - 1, 0
            polys = rng.integers(-(t // 2), t // 2 + 1, size=(3, n), dtype=np.int64)           # the full centred range (-t/2, t/2]
            polys[1, 0], polys[1, n - 1] = t // 2, -(t // 2)
            assert np.array_equal(model.dot_schoolbook(residues, polys, modulus), model.dot_sparse(residues, polys, modulus)), (n, modulus)
    # through combine_row: the header and every component of both blocks
    n, k, moduli = 16, 2, rns_model.rns_moduli(16)
    rows = _rows(rng, 3, n, k, moduli, model.rns_header(n, k, t, moduli))
    words = rng.integers(0, 2**64, size=(3, n), dtype=np.uint64)
    assert np.array_equal(model.combine_row(rows, words, t, n, k, moduli, schoolbook=True), model.combine_row(rows, words, t, n, k, moduli))


def test_centred_words_equals_centred_poly():
    rng = np.random.default_rng(7)
    for t in (rns_model.plain_modulus(2), rns_model.plain_modulus(4096), rns_model.plain_modulus(131072)):
        words = rng.integers(0, 2**64, size=(3, 50), dtype=np.uint64)
        words[0, :8] = [0, 1, t // 2, t // 2 + 1, t - 1, t, t + 5, 2**64 - 1]
        got = model.centred_words(words, t)
        assert got.shape == words.shape and got.dtype == np.int64
        assert np.array_equal(got.ravel(), model.centred_poly(words, t))
        assert int(np.abs(got).sum()) == model.weight(words, t)


def test_folding_the_polynomials_of_shared_rows_keeps_the_combination():
    rng = np.random.default_rng(8)
    n, k, q, t = 32, 1, 17592169062401, rns_model.plain_modulus(4096)
    distinct, terms = 3, 11
    pool = _rows(rng, distinct, n, k, (q,), [8 * (4 + (k + 1) * n), 1, n | (k << 32), q, t])
    polys = np.zeros((terms, n), dtype=np.uint64)
    for i in range(terms):
        polys[i, rng.choice(n, size=3, replace=False)] = rng.choice(np.array([1, t - 1, t + 1, 2, t - 2], dtype=np.uint64), size=3)
    row_of_term = (2 + np.arange(terms)) % distinct
    folded = model.fold_shared_rows(polys, row_of_term, distinct, t)
    assert folded.shape == (distinct, n)
    for r in range(distinct):
        assert model.centred_poly(folded[r], t).tolist() == sum(model.centred_poly(p, t) for p in polys[row_of_term == r]).tolist()
    assert np.array_equal(model.combine_row(pool, folded, t, n, k, (q,)), model.combine_row(pool[row_of_term], polys, t, n, k, (q,)))
