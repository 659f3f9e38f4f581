"""CPU suite: the gadget decomposition calls (lsr_ring_gadget_min_digits, lsr_ntt_ring_decompose / recompose / linf / matvec_gadget
_batch and their _device twins) are declared, exported and mirrored in ctypes; the host-only minimum digit count equals the Python-
integer model (tests/ring_gadget_model.py) and the tables the contract was written against; and the refusals that read no handle
(NULL, then the (b, D) shape rules) come first, in the documented order — checked with fake handles that are never dereferenced.  The
refusals behind them read the context (admissibility under its q) and are checked on the GPU (test_ring_gadget_gpu.py)."""
import ctypes
import os
import re

import pytest

import ring_gadget_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_H = os.path.join(ROOT, "include", "lambda_snark", "batch.h")
# name -> (return type, number of arguments)
SYMBOLS = {
    "lsr_ring_gadget_min_digits": (r"uint64_t", 2),
    "lsr_ntt_ring_decompose_batch": (r"int", 6), "lsr_ntt_ring_decompose_batch_device": (r"int", 7),
    "lsr_ntt_ring_recompose_batch": (r"int", 6), "lsr_ntt_ring_recompose_batch_device": (r"int", 7),
    "lsr_ntt_ring_linf_batch": (r"int", 4), "lsr_ntt_ring_linf_batch_device": (r"int", 5),
    "lsr_ntt_ring_matvec_gadget_batch": (r"int", 6), "lsr_ntt_ring_matvec_gadget_batch_device": (r"int", 7),
}
DIGIT_CALLS = ["lsr_ntt_ring_decompose_batch", "lsr_ntt_ring_recompose_batch", "lsr_ntt_ring_matvec_gadget_batch"]


@pytest.fixture()
def fake(pkg):
    """(library, a buffer address, the address of a handle that is never dereferenced: the checks under test come first)"""
    buf = (ctypes.c_uint64 * 16)()
    handle_buf = (ctypes.c_uint64 * 64)()
    yield pkg._abi.load_library(), ctypes.addressof(buf), ctypes.addressof(handle_buf)
    del buf, handle_buf


def _digit_call(lib, name, device, handle, out, x, count, b, digits):
    if device:
        return getattr(lib, name + "_device")(handle, out, x, count, b, digits, None)
    return getattr(lib, name)(handle, out, x, count, b, digits)


def _linf_call(lib, device, handle, x, count, linf):
    if device:
        return lib.lsr_ntt_ring_linf_batch_device(handle, x, count, linf, None)
    return lib.lsr_ntt_ring_linf_batch(handle, x, count, linf)


def test_batch_h_declares_the_block_after_the_matvec():
    raw = open(BATCH_H).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, (ret, count) in SYMBOLS.items():
        found = re.search(ret + r"\s+" + name + r"\s*\(([^)]*)\)", text)
        assert found, name
        assert len(found.group(1).split(",")) == count, name
    assert text.index("lsr_ntt_ring_matvec_batch_device") < text.index("lsr_ring_gadget_min_digits") < text.index("lsr_sample_gaussian_seeded")
    for word in ("ADMISSIBLE", "off = (B/2) (B^D - 1) / (B - 1)", "UINT64_MAX", "no carry chain", "column c D + d"):
        assert word in raw, word                            # the definitions are the contract and live in the header


def test_library_exports_signatures_and_wrappers(pkg):
    lib = pkg._abi.load_library()
    for name, (_, count) in SYMBOLS.items():
        assert hasattr(lib, name), name
        assert len(pkg._abi.SIGNATURES[name][1]) == count, name
    for cls in (pkg.NttContext, pkg.CyclicNtt):
        for attr in ("ring_decompose", "ring_recompose", "ring_linf"):
            assert hasattr(cls, attr) and hasattr(cls, attr + "_device"), (cls, attr)
    assert hasattr(pkg.RingMatrix, "matvec_gadget") and hasattr(pkg.RingMatrix, "matvec_gadget_device")
    assert "ring_gadget_min_digits" in pkg.__all__


def test_model_reproduces_the_tables():
    for q, row in model.MIN_DIGITS_TABLE.items():
        for b, want in row.items():
            assert model.min_digits(q, b) == want, (q, b)
    assert all(model.min_digits(model.GOLDILOCKS, b) == 0 for b in range(2, 33))


def test_min_digits_equals_the_tables(pkg):
    for q, row in model.MIN_DIGITS_TABLE.items():
        for b, want in row.items():
            assert pkg.ring_gadget_min_digits(q, b) == want, (q, b)


@pytest.mark.parametrize("q", model.MODULI)
def test_min_digits_equals_the_model_at_every_base(pkg, q):
    for b in range(2, 33):
        assert pkg.ring_gadget_min_digits(q, b) == model.min_digits(q, b), (q, b)
    for b in (0, 1, 33, 64, 2**32 - 1):                         # outside [2, 32]: no admissible pair
        assert pkg.ring_gadget_min_digits(q, b) == 0, (q, b)


def test_min_digits_is_minimal_and_admissible():
    """The model's own consistency: D is admissible, D - 1 is not, and every word's digits recompose to its centred value."""
    for q in model.MODULI[:4]:
        for b in (2, 3, 4, 8, 11, 16, 32):
            d = model.min_digits(q, b)
            if d == 0:
                continue
            assert model.admissible(q, b, d) and not model.admissible(q, b, d - 1)
            for x in (0, 1, q // 2, q // 2 + 1, q - 1):
                zs = model.digits_of(x, q, b, d)
                assert all(-(1 << (b - 1)) <= z < (1 << (b - 1)) for z in zs)
                assert sum(z << (b * i) for i, z in enumerate(zs)) == model.centred(x, q)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("name", DIGIT_CALLS)
def test_null_is_refused_first(pkg, fake, device, name):
    lib, p, handle = fake
    for h, out, x in [(None, p, p), (handle, None, p), (handle, p, None)]:
        for count, b, digits in [(1, 4, 4), (0, 4, 4), (1, 1, 0), (0, 40, 99)]:      # bad shapes and count == 0 do not come first
            assert _digit_call(lib, name, device, h, out, x, count, b, digits) == -1
            msg = pkg._abi.last_error()
            assert "NULL" in msg and name in msg, msg


@pytest.mark.parametrize("device", [False, True])
def test_linf_refuses_null_and_takes_an_empty_call(pkg, fake, device):
    lib, p, handle = fake
    for h, x, linf in [(None, p, p), (handle, None, p), (handle, p, None)]:
        for count in (1, 0):
            assert _linf_call(lib, device, h, x, count, linf) == -1
            assert "NULL" in pkg._abi.last_error() and "lsr_ntt_ring_linf_batch" in pkg._abi.last_error()
    assert _linf_call(lib, device, handle, p, 0, p) == 0          # (the fake context is not read)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("name", DIGIT_CALLS)
def test_shape_rules_come_before_anything_that_reads_the_handle(pkg, fake, device, name):
    """b outside [2, 32], then D == 0, then b D > 64 (recompose: b (D - 1) > 64) — also for count == 0 and overlapping buffers, which
    are looked at later.  The handle is fake: reading it would crash or give nonsense, not these messages."""
    lib, p, handle = fake
    recompose = "recompose" in name
    cases = [(0, 4, "base_log2"), (1, 4, "base_log2"), (33, 1, "base_log2"), (33, 0, "base_log2"), (4, 0, "digits must be at least 1"),
             (32, 0, "digits must be at least 1")]
    over = [(4, 18), (32, 4), (2, 34), (22, 4)] if recompose else [(4, 17), (32, 3), (2, 33), (22, 3)]
    cases += [(b, d, "above 64") for b, d in over]
    for b, digits, named in cases:
        for count in (1, 0):
            assert _digit_call(lib, name, device, handle, p, p, count, b, digits) == -1, (b, digits)
            msg = pkg._abi.last_error()
            assert named in msg and name in msg, (b, digits, msg)


@pytest.mark.parametrize("device", [False, True])
def test_recompose_takes_one_digit_more_than_decompose_and_an_empty_call(pkg, fake, device):
    """b (D - 1) <= 64 is all recompose asks: (4, 17), (32, 3) and (2, 33) pass its shape rules, and with count == 0 the call is a no-op
    that never reads the (fake) context."""
    lib, p, handle = fake
    for b, digits in [(4, 17), (32, 3), (2, 33), (4, 1), (32, 1)]:
        assert _digit_call(lib, "lsr_ntt_ring_recompose_batch", device, handle, p, p, 0, b, digits) == 0, (b, digits)
