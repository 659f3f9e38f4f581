"""CPU suite: the Galois automorphisms and the twisted ring inner product (lsr_ntt_ring_automorphism_batch / _device,
lsr_ntt_ring_dot_galois_batch / _device) are declared, exported and mirrored in ctypes, the Python members exist on both context
classes, and the argument checks that read no context run before any device work, in batch.h's order — so they answer -1 with a
message on a machine without a GPU, given a handle that is never dereferenced."""
import ctypes
import os
import re

import pytest

from ring_galois_model import (test_automorphism_by_hand,  # noqa: F401  (collected here: the model's own tests)
                               test_automorphism_is_a_ring_homomorphism_and_a_group_action)  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_H = os.path.join(ROOT, "include", "lambda_snark", "batch.h")
AUTO, AUTO_DEV = "lsr_ntt_ring_automorphism_batch", "lsr_ntt_ring_automorphism_batch_device"
DOT, DOT_DEV = "lsr_ntt_ring_dot_galois_batch", "lsr_ntt_ring_dot_galois_batch_device"
ARGUMENTS = {
    AUTO: ["ctx", "out", "x", "count", "g"],
    AUTO_DEV: ["ctx", "d_out", "d_x", "count", "g", "stream"],
    DOT: ["ctx", "c", "a", "b", "batch", "terms", "b_rows", "g"],
    DOT_DEV: ["ctx", "d_c", "d_a", "d_b", "batch", "terms", "b_rows", "g", "stream"],
}
SIZE_MAX = (1 << (8 * ctypes.sizeof(ctypes.c_size_t))) - 1
EVEN = [0, 2, 4096, (1 << 64) - 2]


def _auto(lib, device, ctx, out, x, count, g):
    if device:
        return lib.lsr_ntt_ring_automorphism_batch_device(ctx, out, x, count, g, None)
    return lib.lsr_ntt_ring_automorphism_batch(ctx, out, x, count, g)


def _dot(lib, device, ctx, c, a, b, batch, terms, b_rows, g):
    if device:
        return lib.lsr_ntt_ring_dot_galois_batch_device(ctx, c, a, b, batch, terms, b_rows, g, None)
    return lib.lsr_ntt_ring_dot_galois_batch(ctx, c, a, b, batch, terms, b_rows, g)


@pytest.fixture()
def fake(pkg):
    """(library, a buffer address, the address of a context that is never dereferenced: the checks come first)"""
    buf = (ctypes.c_uint64 * 16)()
    ctx_buf = (ctypes.c_uint64 * 64)()
    yield pkg._abi.load_library(), ctypes.addressof(buf), ctypes.addressof(ctx_buf)
    del buf, ctx_buf


def test_batch_h_declares_the_four_functions():
    text = re.sub(r"/\*.*?\*/", "", open(BATCH_H).read(), flags=re.S)
    for name, want in ARGUMENTS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
        assert m, name
        assert [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")] == want, name


def test_library_exports_signatures_and_members(pkg):
    lib = pkg._abi.load_library()
    for name, want in ARGUMENTS.items():
        assert hasattr(lib, name), name
        assert name in pkg._abi.SIGNATURES, name
        assert len(pkg._abi.SIGNATURES[name][1]) == len(want), name
    assert [len(pkg._abi.SIGNATURES[name][1]) for name in (AUTO, AUTO_DEV, DOT, DOT_DEV)] == [5, 6, 8, 9]
    for cls in (pkg.NttContext, pkg.CyclicNtt):
        for member in ("ring_automorphism", "ring_automorphism_device", "ring_dot_galois", "ring_dot_galois_device"):
            assert callable(getattr(cls, member)), (cls, member)
        assert isinstance(cls.galois_conjugation, property), cls


@pytest.mark.parametrize("device", [False, True])
def test_null_arguments_are_refused_first(pkg, fake, device):
    lib, b, fake_ctx = fake
    # (the later checks would fail too — an even g, b_rows, no terms: NULL is reported first)
    for ctx, out, x in [(None, b, b), (fake_ctx, None, b), (fake_ctx, b, None)]:
        for count, g in [(1, 1), (0, 1), (3, 2), (SIZE_MAX, 0)]:
            assert _auto(lib, device, ctx, out, x, count, g) == -1
            msg = pkg._abi.last_error()
            assert "NULL" in msg and (AUTO_DEV if device else AUTO) + ":" in msg
    for ctx, c, a, bb in [(None, b, b, b), (fake_ctx, None, b, b), (fake_ctx, b, None, b), (fake_ctx, b, b, None)]:
        for batch, terms, b_rows, g in [(1, 1, 1, 1), (3, 0, 2, 2), (0, 1, 0, 0)]:
            assert _dot(lib, device, ctx, c, a, bb, batch, terms, b_rows, g) == -1
            msg = pkg._abi.last_error()
            assert "NULL" in msg and (DOT_DEV if device else DOT) + ":" in msg


@pytest.mark.parametrize("device", [False, True])
def test_b_rows_then_terms_are_refused_before_g(pkg, fake, device):
    lib, b, fake_ctx = fake
    for g in [1, 2, 0]:
        assert _dot(lib, device, fake_ctx, b, b, b, 3, 0, 2, g) == -1          # b_rows before terms
        assert "b_rows" in pkg._abi.last_error()
        assert _dot(lib, device, fake_ctx, b, b, b, 0, 0, 2, g) == -1          # (batch = 0 takes b_rows 1 or 0, and is not a no-op yet)
        assert "b_rows" in pkg._abi.last_error()
        for batch, b_rows in [(3, 3), (3, 1), (0, 0)]:
            assert _dot(lib, device, fake_ctx, b, b, b, batch, 0, b_rows, g) == -1
            msg = pkg._abi.last_error()
            assert "terms" in msg and "b_rows" not in msg and "even" not in msg


@pytest.mark.parametrize("device", [False, True])
def test_even_g_is_refused_before_the_empty_call(pkg, fake, device):
    lib, b, fake_ctx = fake
    for g in EVEN:
        for count in [0, 1, 5, SIZE_MAX]:
            assert _auto(lib, device, fake_ctx, b, b, count, g) == -1, (count, g)
            msg = pkg._abi.last_error()
            assert "g = " + str(g) in msg and "even" in msg and (AUTO_DEV if device else AUTO) + ":" in msg
        for batch, terms, b_rows in [(0, 1, 0), (0, 3, 1), (2, 3, 2), (SIZE_MAX, SIZE_MAX, 1)]:
            assert _dot(lib, device, fake_ctx, b, b, b, batch, terms, b_rows, g) == -1, (batch, g)
            msg = pkg._abi.last_error()
            assert "g = " + str(g) in msg and "even" in msg and (DOT_DEV if device else DOT) + ":" in msg


@pytest.mark.parametrize("device", [False, True])
def test_empty_calls_are_no_ops_with_an_odd_g(pkg, fake, device):
    lib, b, fake_ctx = fake
    # 0, whatever the later checks would say: g above every N, terms above the cap, products that overflow
    for g in [1, 3, (1 << 23) + 1, (1 << 64) - 1]:
        assert _auto(lib, device, fake_ctx, b, b, 0, g) == 0
        for terms, b_rows in [(1, 0), (1, 1), (1 << 20, 1), (SIZE_MAX, 1)]:
            assert _dot(lib, device, fake_ctx, b, b, b, 0, terms, b_rows, g) == 0


@pytest.mark.parametrize("device", [False, True])
def test_overflowing_sizes_are_refused(pkg, fake, device):
    lib, b, fake_ctx = fake
    half = 1 << (4 * ctypes.sizeof(ctypes.c_size_t))          # half * half wraps to 0
    for count in [SIZE_MAX // 16 + 1, SIZE_MAX]:              # bytes of the smallest ring
        assert _auto(lib, device, fake_ctx, b, b, count, 1) == -1, count
        msg = pkg._abi.last_error()
        assert "overflow" in msg and (AUTO_DEV if device else AUTO) + ":" in msg
    cases = [
        (half, half, half),                 # batch * terms
        (SIZE_MAX // 2, 4, 1),              # batch * terms
        (SIZE_MAX // 16 + 1, 1, 1),         # bytes of c (and a) at the smallest ring
        (SIZE_MAX // 64 + 1, 4, 1),         # bytes of a at the smallest ring
    ]
    for batch, terms, b_rows in cases:
        assert _dot(lib, device, fake_ctx, b, b, b, batch, terms, b_rows, 3) == -1, (batch, terms, b_rows)
        msg = pkg._abi.last_error()
        assert "overflow" in msg and (DOT_DEV if device else DOT) + ":" in msg
