"""CPU suite: the ring quadratic forms and the symmetrised packed Gram matrix (lsr_ntt_ring_quadform_batch, lsr_ntt_ring_gram_sym2_batch
and their _device forms) are declared, exported and mirrored in ctypes, the Python members exist on both context
classes, and the argument checks that read no context run before any device work, in batch.h's order — so they answer -1 with a
message on a machine without a GPU, given a handle that is never dereferenced."""
import ctypes
import os
import re

import pytest

from ring_quadform_model import (test_flat_spectrum_closed_forms_equal_schoolbook,  # noqa: F401  (collected here: the model's own tests)
                                 test_oracle_references_equal_schoolbook,  # noqa: F401
                                 test_quadform_by_hand,  # noqa: F401
                                 test_quadform_of_a_gram_matrix_is_the_norm_of_the_fold,  # noqa: F401
                                 test_sym2_is_the_cross_form_plus_its_transpose)  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_H = os.path.join(ROOT, "include", "lambda_snark", "batch.h")
QUAD, SYM2 = "lsr_ntt_ring_quadform_batch", "lsr_ntt_ring_gram_sym2_batch"
ARGUMENTS = {
    QUAD: ["ctx", "out", "g", "c", "batch", "r", "c_rows", "offdiag"],
    QUAD + "_device": ["ctx", "d_out", "d_g", "d_c", "batch", "r", "c_rows", "offdiag", "stream"],
    SYM2: ["ctx", "h", "a", "b", "batch", "r", "width"],
    SYM2 + "_device": ["ctx", "d_h", "d_a", "d_b", "batch", "r", "width", "stream"],
}
SIZE_MAX = (1 << (8 * ctypes.sizeof(ctypes.c_size_t))) - 1
HALF = 1 << (4 * ctypes.sizeof(ctypes.c_size_t))          # HALF * HALF wraps to 0
MAX_VECTORS, MAX_TERMS = 64, 65536


def _name(base, device):
    return base + "_device" if device else base


def _quad(lib, device, ctx, out, g, c, batch, r, c_rows, offdiag=2):
    if device:
        return lib.lsr_ntt_ring_quadform_batch_device(ctx, out, g, c, batch, r, c_rows, offdiag, None)
    return lib.lsr_ntt_ring_quadform_batch(ctx, out, g, c, batch, r, c_rows, offdiag)


def _sym2(lib, device, ctx, h, a, b, batch, r, width):
    if device:
        return lib.lsr_ntt_ring_gram_sym2_batch_device(ctx, h, a, b, batch, r, width, None)
    return lib.lsr_ntt_ring_gram_sym2_batch(ctx, h, a, b, batch, r, width)


@pytest.fixture()
def fake(pkg):
    """(library, a buffer address, the address of a context that is never dereferenced: the checks come first)"""
    buf = (ctypes.c_uint64 * 16)()
    ctx_buf = (ctypes.c_uint64 * 64)()
    yield pkg._abi.load_library(), ctypes.addressof(buf), ctypes.addressof(ctx_buf)
    del buf, ctx_buf


def test_batch_h_declares_the_functions_with_their_argument_names():
    text = re.sub(r"/\*.*?\*/", "", open(BATCH_H).read(), flags=re.S)
    for name, want in ARGUMENTS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
        assert m, name
        assert [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")] == want, name
    assert re.search(r"uint64_t\s+offdiag", text)


def test_library_exports_signatures_and_members(pkg):
    lib = pkg._abi.load_library()
    for name, want in ARGUMENTS.items():
        assert hasattr(lib, name), name
        assert len(pkg._abi.SIGNATURES[name][1]) == len(want), name
    for cls in (pkg.NttContext, pkg.CyclicNtt):
        for member in ("ring_quadform", "ring_quadform_device", "ring_gram_sym2", "ring_gram_sym2_device"):
            assert callable(getattr(cls, member)), member


# ---- the quadratic form: refusals (1) - (5) ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True])
def test_quadform_null_arguments_are_refused_first(pkg, fake, device):
    lib, b, ctx = fake
    # (the later checks would fail too — r == 0, c_rows neither 1 nor batch, r above the cap, overflowing sizes: NULL is reported first)
    for c, out, g, cc in [(None, b, b, b), (ctx, None, b, b), (ctx, b, None, b), (ctx, b, b, None)]:
        for batch, r, c_rows in [(1, 1, 1), (0, 0, 0), (2, 0, 5), (3, MAX_VECTORS + 1, 2), (SIZE_MAX, SIZE_MAX, SIZE_MAX)]:
            assert _quad(lib, device, c, out, g, cc, batch, r, c_rows) == -1
            msg = pkg._abi.last_error()
            assert "NULL" in msg and _name(QUAD, device) + ":" in msg


@pytest.mark.parametrize("device", [False, True])
def test_quadform_zero_r_then_c_rows_then_the_cap_then_overflow(pkg, fake, device):
    lib, b, ctx = fake
    # (2) r == 0, before the c_rows rule
    for batch, c_rows in [(0, 0), (1, 1), (4, 2), (SIZE_MAX, 7)]:
        assert _quad(lib, device, ctx, b, b, b, batch, 0, c_rows) == -1
        msg = pkg._abi.last_error()
        assert "at least 1" in msg and _name(QUAD, device) + ":" in msg
    # (3) c_rows neither 1 nor batch, before the cap
    for batch, r, c_rows in [(4, 2, 2), (0, 2, 3), (3, MAX_VECTORS + 1, 2), (SIZE_MAX, SIZE_MAX, 2), (2, HALF, 0)]:
        assert _quad(lib, device, ctx, b, b, b, batch, r, c_rows) == -1, (batch, r, c_rows)
        msg = pkg._abi.last_error()
        assert "c_rows" in msg and "MAX" not in msg and _name(QUAD, device) + ":" in msg
    # (4) the cap, before the overflowing products
    for batch, r, c_rows in [(1, MAX_VECTORS + 1, 1), (0, MAX_VECTORS + 1, 0), (SIZE_MAX, SIZE_MAX, SIZE_MAX), (HALF, HALF, HALF), (SIZE_MAX, HALF, 1)]:
        assert _quad(lib, device, ctx, b, b, b, batch, r, c_rows) == -1, (batch, r, c_rows)
        msg = pkg._abi.last_error()
        assert "LSR_RING_GRAM_MAX_VECTORS" in msg and "overflow" not in msg and _name(QUAD, device) + ":" in msg
    # (5) batch * pairs, c_rows * r, and each times 16 bytes
    pairs = MAX_VECTORS * (MAX_VECTORS + 1) // 2
    for batch, r, c_rows in [(SIZE_MAX, 2, SIZE_MAX), (SIZE_MAX, 2, 1), (SIZE_MAX // pairs + 1, MAX_VECTORS, 1), (SIZE_MAX // 16 + 1, 1, 1),
                             (SIZE_MAX // 48 + 1, 2, 1), (SIZE_MAX // 32 + 1, 2, SIZE_MAX // 32 + 1)]:
        assert _quad(lib, device, ctx, b, b, b, batch, r, c_rows) == -1, (batch, r, c_rows)
        msg = pkg._abi.last_error()
        assert "overflow" in msg and _name(QUAD, device) + ":" in msg


@pytest.mark.parametrize("device", [False, True])
def test_quadform_empty_batch_is_a_no_op_and_the_cap_itself_is_allowed(pkg, fake, device):
    lib, b, ctx = fake
    # 0, whatever the checks that read the context would say: offdiag above every modulus, out on top of g and c, a context of zeros
    for r in (1, 5, MAX_VECTORS):
        for c_rows in (0, 1):
            for offdiag in (0, 2, (1 << 64) - 1):
                assert _quad(lib, device, ctx, b, b, b, 0, r, c_rows, offdiag) == 0, (r, c_rows, offdiag)


# ---- the symmetrised Gram matrix: the Gram call's refusals with ra = rb = r, and a NULL b ---------------------------------------------------
@pytest.mark.parametrize("device", [False, True])
def test_sym2_null_arguments_are_refused_first_b_included(pkg, fake, device):
    lib, b, ctx = fake
    for c, h, a, bb in [(None, b, b, b), (ctx, None, b, b), (ctx, b, None, b), (ctx, b, b, None)]:
        for batch, r, width in [(1, 1, 1), (0, 0, 0), (0, 2, 2), (1, MAX_VECTORS + 1, MAX_TERMS + 1), (SIZE_MAX, SIZE_MAX, SIZE_MAX)]:
            assert _sym2(lib, device, c, h, a, bb, batch, r, width) == -1
            msg = pkg._abi.last_error()
            assert "NULL" in msg and _name(SYM2, device) + ":" in msg


@pytest.mark.parametrize("device", [False, True])
def test_sym2_zero_sizes_then_the_caps_then_overflow(pkg, fake, device):
    lib, b, ctx = fake
    for batch, r, width in [(1, 0, 1), (1, 1, 0), (0, 0, 0), (SIZE_MAX, 0, SIZE_MAX), (1, MAX_VECTORS + 1, 0)]:
        assert _sym2(lib, device, ctx, b, b, b, batch, r, width) == -1
        msg = pkg._abi.last_error()
        assert "at least 1" in msg and _name(SYM2, device) + ":" in msg
    for batch, r, width in [(1, MAX_VECTORS + 1, 1), (0, MAX_VECTORS + 1, 1), (SIZE_MAX, SIZE_MAX, SIZE_MAX), (HALF, HALF, HALF)]:
        assert _sym2(lib, device, ctx, b, b, b, batch, r, width) == -1
        msg = pkg._abi.last_error()
        assert "LSR_RING_GRAM_MAX_VECTORS" in msg and "overflow" not in msg and _name(SYM2, device) + ":" in msg
    for batch, width in [(0, MAX_TERMS + 1), (1, MAX_TERMS + 1), (HALF, HALF), (SIZE_MAX, SIZE_MAX)]:
        assert _sym2(lib, device, ctx, b, b, b, batch, 2, width) == -1
        msg = pkg._abi.last_error()
        assert "LSR_RING_DOT_MAX_TERMS" in msg and "overflow" not in msg and _name(SYM2, device) + ":" in msg
    # batch * r * width, batch * r (r + 1) / 2, and each times 16 bytes: r = 3 has 6 outputs, twice its 3 operand polynomials at width 1
    for batch, r, width in [(SIZE_MAX, 2, 1), (SIZE_MAX, 1, 2), (1 << 44, MAX_VECTORS, MAX_TERMS), (SIZE_MAX // 16 + 1, 1, 1), (SIZE_MAX // 96 + 1, 3, 1),
                            (SIZE_MAX // 48 + 1, 1, 3)]:
        assert _sym2(lib, device, ctx, b, b, b, batch, r, width) == -1, (batch, r, width)
        msg = pkg._abi.last_error()
        assert "overflow" in msg and _name(SYM2, device) + ":" in msg


@pytest.mark.parametrize("device", [False, True])
def test_sym2_empty_batch_is_a_no_op_and_the_caps_themselves_are_allowed(pkg, fake, device):
    lib, b, ctx = fake
    for r, width in [(1, 1), (3, 5), (MAX_VECTORS, MAX_TERMS)]:
        assert _sym2(lib, device, ctx, b, b, b, 0, r, width) == 0
