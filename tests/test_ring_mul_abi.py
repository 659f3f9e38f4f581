"""CPU suite: the batched ring multiply (lsr_ntt_ring_mul_batch / _device) is declared, exported and mirrored in ctypes, and its
argument checks run before any device work — so they answer -1 with a message on a machine without a GPU."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_H = os.path.join(ROOT, "include", "lambda_snark", "batch.h")
SYMBOLS = ["lsr_ntt_ring_mul_batch", "lsr_ntt_ring_mul_batch_device"]


def test_batch_h_declares_the_ring_multiply():
    text = re.sub(r"/\*.*?\*/", "", open(BATCH_H).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name


def test_library_exports_and_signatures(pkg):
    lib = pkg._abi.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in pkg._abi.SIGNATURES, name
    assert len(pkg._abi.SIGNATURES["lsr_ntt_ring_mul_batch"][1]) == 6
    assert len(pkg._abi.SIGNATURES["lsr_ntt_ring_mul_batch_device"][1]) == 7
    assert hasattr(pkg.NttContext, "ring_mul") and hasattr(pkg.NttContext, "ring_mul_device")
    assert hasattr(pkg.CyclicNtt, "ring_mul") and hasattr(pkg.CyclicNtt, "ring_mul_device")


@pytest.mark.parametrize("device", [False, True])
def test_null_arguments_are_refused(pkg, device):
    lib = pkg._abi.load_library()
    buf = (ctypes.c_uint64 * 16)()
    p = ctypes.addressof(buf)
    ctx_buf = (ctypes.c_uint64 * 64)()
    fake_ctx = ctypes.addressof(ctx_buf)   # never dereferenced: the checks come first
    for ctx, c, a, b in [(None, p, p, p), (fake_ctx, None, p, p), (fake_ctx, p, None, p), (fake_ctx, p, p, None)]:
        if device:
            rc = lib.lsr_ntt_ring_mul_batch_device(ctx, c, a, b, 1, 1, None)
        else:
            rc = lib.lsr_ntt_ring_mul_batch(ctx, c, a, b, 1, 1)
        assert rc == -1
        msg = pkg._abi.last_error()
        assert msg and "NULL" in msg


@pytest.mark.parametrize("device", [False, True])
def test_b_rows_must_be_one_or_batch(pkg, device):
    lib = pkg._abi.load_library()
    buf = (ctypes.c_uint64 * 16)()
    p = ctypes.addressof(buf)
    ctx_buf = (ctypes.c_uint64 * 64)()
    fake_ctx = ctypes.addressof(ctx_buf)
    for batch, b_rows in [(3, 2), (3, 0), (1, 2), (0, 5)]:
        if device:
            rc = lib.lsr_ntt_ring_mul_batch_device(fake_ctx, p, p, p, batch, b_rows, None)
        else:
            rc = lib.lsr_ntt_ring_mul_batch(fake_ctx, p, p, p, batch, b_rows)
        assert rc == -1
        assert "b_rows" in pkg._abi.last_error()
