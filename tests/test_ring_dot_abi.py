"""CPU suite: the batched ring inner product (lsr_ntt_ring_dot_batch / _device) is declared, exported and mirrored in ctypes, and its
argument checks run before any device work, in the documented order — so they answer -1 with a message on a machine without a GPU."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_H = os.path.join(ROOT, "include", "lambda_snark", "batch.h")
SYMBOLS = ["lsr_ntt_ring_dot_batch", "lsr_ntt_ring_dot_batch_device"]


def _call(lib, device, ctx, c, a, b, batch, terms, b_rows):
    if device:
        return lib.lsr_ntt_ring_dot_batch_device(ctx, c, a, b, batch, terms, b_rows, None)
    return lib.lsr_ntt_ring_dot_batch(ctx, c, a, b, batch, terms, b_rows)


@pytest.fixture()
def fake(pkg):
    """(library, a buffer address, the address of a context that is never dereferenced: the checks come first)"""
    buf = (ctypes.c_uint64 * 16)()
    ctx_buf = (ctypes.c_uint64 * 64)()
    yield pkg._abi.load_library(), ctypes.addressof(buf), ctypes.addressof(ctx_buf)
    del buf, ctx_buf


def test_batch_h_declares_the_ring_inner_product():
    raw = open(BATCH_H).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
    assert re.search(r"#define\s+LSR_RING_DOT_MAX_TERMS\s+\d+", text)          # the cap on terms is stated in the header
    assert re.search(r"#define\s+LSR_RING_DOT_F64_RECENTRE_PERIOD\s+\d+", text)


def test_library_exports_and_signatures(pkg):
    lib = pkg._abi.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in pkg._abi.SIGNATURES, name
    assert len(pkg._abi.SIGNATURES["lsr_ntt_ring_dot_batch"][1]) == 7
    assert len(pkg._abi.SIGNATURES["lsr_ntt_ring_dot_batch_device"][1]) == 8
    assert hasattr(pkg.NttContext, "ring_dot") and hasattr(pkg.NttContext, "ring_dot_device")
    assert hasattr(pkg.CyclicNtt, "ring_dot") and hasattr(pkg.CyclicNtt, "ring_dot_device")


def test_python_constants_mirror_the_header(pkg):
    text = open(BATCH_H).read()
    assert int(re.search(r"#define\s+LSR_RING_DOT_F64_RECENTRE_PERIOD\s+(\d+)", text).group(1)) == pkg.RING_DOT_F64_RECENTRE_PERIOD
    assert int(re.search(r"#define\s+LSR_RING_DOT_MAX_TERMS\s+(\d+)", text).group(1)) == pkg.RING_DOT_MAX_TERMS
    assert pkg.RING_DOT_MAX_TERMS >= 4096


@pytest.mark.parametrize("device", [False, True])
def test_null_arguments_are_refused(pkg, fake, device):
    lib, p, fake_ctx = fake
    # (the later checks would fail too — b_rows = 2, terms = 0: NULL is reported first)
    for ctx, c, a, b in [(None, p, p, p), (fake_ctx, None, p, p), (fake_ctx, p, None, p), (fake_ctx, p, p, None)]:
        for batch, terms, b_rows in [(1, 1, 1), (3, 0, 2)]:
            assert _call(lib, device, ctx, c, a, b, batch, terms, b_rows) == -1
            msg = pkg._abi.last_error()
            assert msg and "NULL" in msg


@pytest.mark.parametrize("device", [False, True])
def test_b_rows_must_be_one_or_batch(pkg, fake, device):
    lib, p, fake_ctx = fake
    # terms = 0 among them: b_rows is reported before terms, and before the batch == 0 no-op
    for batch, terms, b_rows in [(3, 2, 2), (3, 1, 0), (1, 4, 2), (0, 1, 5), (3, 0, 2)]:
        assert _call(lib, device, fake_ctx, p, p, p, batch, terms, b_rows) == -1
        assert "b_rows" in pkg._abi.last_error()


@pytest.mark.parametrize("device", [False, True])
def test_zero_terms_are_refused(pkg, fake, device):
    lib, p, fake_ctx = fake
    for batch, b_rows in [(3, 3), (3, 1), (1, 1), (0, 0), (0, 1)]:      # batch == 0 is a no-op only after this check
        assert _call(lib, device, fake_ctx, p, p, p, batch, 0, b_rows) == -1
        msg = pkg._abi.last_error()
        assert "terms" in msg and "b_rows" not in msg


@pytest.mark.parametrize("device", [False, True])
def test_empty_batch_is_a_no_op(pkg, fake, device):
    lib, p, fake_ctx = fake
    for terms, b_rows in [(1, 0), (7, 1)]:
        assert _call(lib, device, fake_ctx, p, p, p, 0, terms, b_rows) == 0
