"""CPU suite: the ring Gram matrices (lsr_ntt_ring_gram_batch, its _device form and lsr_ntt_ring_gram_block) are declared, exported and
mirrored in ctypes, the Python members exist on both context classes, and the argument checks that read no context run before any
device work, in batch.h's order — so they answer -1 with a message on a machine without a GPU, given a handle that is never
dereferenced."""
import ctypes
import os
import re

import pytest

from ring_gram_model import (test_gram_by_hand,  # noqa: F401  (collected here: the model's own tests)
                             test_oracle_gram_equals_schoolbook,  # noqa: F401
                             test_packed_index_matches_enumeration,  # noqa: F401
                             test_symmetric_form_is_the_upper_triangle_of_the_cross_form)  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_H = os.path.join(ROOT, "include", "lambda_snark", "batch.h")
GRAM = "lsr_ntt_ring_gram_batch"
ARGUMENTS = {
    GRAM: ["ctx", "g", "a", "b", "batch", "ra", "rb", "width"],
    GRAM + "_device": ["ctx", "d_g", "d_a", "d_b", "batch", "ra", "rb", "width", "stream"],
}
SIZE_MAX = (1 << (8 * ctypes.sizeof(ctypes.c_size_t))) - 1
HALF = 1 << (4 * ctypes.sizeof(ctypes.c_size_t))          # HALF * HALF wraps to 0
MAX_VECTORS, MAX_TERMS = 64, 65536


def _name(device):
    return GRAM + "_device" if device else GRAM


def _gram(lib, device, ctx, g, a, b, batch, ra, rb, width):
    if device:
        return lib.lsr_ntt_ring_gram_batch_device(ctx, g, a, b, batch, ra, rb, width, None)
    return lib.lsr_ntt_ring_gram_batch(ctx, g, a, b, batch, ra, rb, width)


@pytest.fixture()
def fake(pkg):
    """(library, a buffer address, the address of a context that is never dereferenced: the checks come first)"""
    buf = (ctypes.c_uint64 * 16)()
    ctx_buf = (ctypes.c_uint64 * 64)()
    yield pkg._abi.load_library(), ctypes.addressof(buf), ctypes.addressof(ctx_buf)
    del buf, ctx_buf


def test_batch_h_declares_the_functions_and_both_macros():
    raw = open(BATCH_H).read()
    assert re.search(r"#define\s+LSR_RING_GRAM_MAX_VECTORS\s+64\b", raw)
    assert re.search(r"#define\s+LSR_RING_GRAM_MAX_FAMILY_BYTES\s+1073741824\b", raw)
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, want in ARGUMENTS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
        assert m, name
        assert [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")] == want, name
    m = re.search(r"\bsize_t\s+lsr_ntt_ring_gram_block\s*\(([^)]*)\)", text)
    assert m and m.group(1).split()[-1].lstrip("*") == "ctx"


def test_library_exports_signatures_and_members(pkg):
    lib = pkg._abi.load_library()
    for name, want in ARGUMENTS.items():
        assert hasattr(lib, name), name
        assert len(pkg._abi.SIGNATURES[name][1]) == len(want), name
    assert hasattr(lib, "lsr_ntt_ring_gram_block") and len(pkg._abi.SIGNATURES["lsr_ntt_ring_gram_block"][1]) == 1
    assert lib.lsr_ntt_ring_gram_block(None) == 0
    assert pkg.RING_GRAM_MAX_VECTORS == MAX_VECTORS and pkg.RING_DOT_MAX_TERMS == MAX_TERMS
    for cls in (pkg.NttContext, pkg.CyclicNtt):
        assert callable(cls.ring_gram) and callable(cls.ring_gram_device)
        assert isinstance(cls.ring_gram_block, property)
    assert [pkg.ring_gram_index(3, i, l) for i in range(3) for l in range(i, 3)] == list(range(6))
    with pytest.raises(ValueError):
        pkg.ring_gram_index(3, 2, 1)


@pytest.mark.parametrize("device", [False, True])
def test_null_arguments_are_refused_first(pkg, fake, device):
    lib, b, ctx = fake
    # (the later checks would fail too — zero sizes, rb != ra, sizes above the caps, overflowing sizes: NULL is reported first)
    for c, g, a in [(None, b, b), (ctx, None, b), (ctx, b, None)]:
        for other in (b, None):
            for batch, ra, rb, width in [(1, 1, 1, 1), (0, 0, 0, 0), (1, 2, 3, 1), (SIZE_MAX, SIZE_MAX, SIZE_MAX, SIZE_MAX)]:
                assert _gram(lib, device, c, g, a, other, batch, ra, rb, width) == -1
                msg = pkg._abi.last_error()
                assert "NULL" in msg and _name(device) + ":" in msg


@pytest.mark.parametrize("device", [False, True])
def test_zero_sizes_then_the_symmetric_rule_then_the_caps(pkg, fake, device):
    lib, b, ctx = fake
    # (2) zero sizes, before the symmetric rule and the caps
    for other, ra, rb, width in [(b, 0, 1, 1), (b, 1, 0, 1), (b, 1, 1, 0), (None, 0, 0, 1), (None, 0, 3, 1), (None, 2, 3, 0), (b, 0, SIZE_MAX, SIZE_MAX)]:
        for batch in (0, 1, SIZE_MAX):
            assert _gram(lib, device, ctx, b, b, other, batch, ra, rb, width) == -1, (ra, rb, width)
            msg = pkg._abi.last_error()
            assert "at least 1" in msg and _name(device) + ":" in msg
    # (3) rb != ra with NULL b, before the caps (rb = 0 included: rb is not a size of the symmetric form)
    for ra, rb, width in [(2, 3, 1), (3, 0, 1), (1, SIZE_MAX, 1), (SIZE_MAX, 1, SIZE_MAX), (MAX_VECTORS + 1, MAX_VECTORS + 2, MAX_TERMS + 1)]:
        for batch in (0, 1, SIZE_MAX):
            assert _gram(lib, device, ctx, b, b, None, batch, ra, rb, width) == -1, (ra, rb)
            msg = pkg._abi.last_error()
            assert "rb == ra" in msg and "MAX" not in msg and _name(device) + ":" in msg
    # (4) the caps, before the overflowing products
    for other, ra, rb in [(b, MAX_VECTORS + 1, 1), (b, 1, MAX_VECTORS + 1), (None, MAX_VECTORS + 1, MAX_VECTORS + 1), (b, HALF, HALF), (b, SIZE_MAX, 2),
                          (None, HALF, HALF)]:
        for batch, width in [(0, 1), (1, 1), (SIZE_MAX, SIZE_MAX), (HALF, HALF)]:
            assert _gram(lib, device, ctx, b, b, other, batch, ra, rb, width) == -1, (ra, rb)
            msg = pkg._abi.last_error()
            assert "LSR_RING_GRAM_MAX_VECTORS" in msg and "overflow" not in msg and _name(device) + ":" in msg
    for batch, width in [(0, MAX_TERMS + 1), (1, MAX_TERMS + 1), (HALF, HALF), (2, SIZE_MAX), (SIZE_MAX, SIZE_MAX)]:
        for other in (b, None):
            assert _gram(lib, device, ctx, b, b, other, batch, 2, 2, width) == -1, (batch, width)
            msg = pkg._abi.last_error()
            assert "LSR_RING_DOT_MAX_TERMS" in msg and "overflow" not in msg and _name(device) + ":" in msg
    # the caps themselves are allowed: batch == 0 gets past every check that reads no context
    assert _gram(lib, device, ctx, b, b, b, 0, MAX_VECTORS, MAX_VECTORS, MAX_TERMS) == 0
    assert _gram(lib, device, ctx, b, b, None, 0, MAX_VECTORS, MAX_VECTORS, MAX_TERMS) == 0


@pytest.mark.parametrize("device", [False, True])
def test_overflowing_sizes_are_refused(pkg, fake, device):
    lib, b, ctx = fake
    # batch * ra * width, batch * rb * width, batch * outputs, and each times 16 bytes (the smallest ring)
    cases = [(SIZE_MAX, 2, 1, 1), (SIZE_MAX, 1, 2, 1), (SIZE_MAX, 1, 1, 2), (1 << 44, MAX_VECTORS, 1, MAX_TERMS), (1 << 44, 1, MAX_VECTORS, MAX_TERMS),
             (SIZE_MAX // 16 + 1, 1, 1, 1), (SIZE_MAX // 32 + 1, 2, 1, 1), (SIZE_MAX // 32 + 1, 1, 2, 1), (SIZE_MAX // 64 + 1, 2, 2, 1),
             (SIZE_MAX // 64 + 1, 1, 1, 4)]
    for batch, ra, rb, width in cases:
        assert _gram(lib, device, ctx, b, b, b, batch, ra, rb, width) == -1, (batch, ra, rb, width)
        msg = pkg._abi.last_error()
        assert "overflow" in msg and _name(device) + ":" in msg
    # symmetric: r = 3 has 6 outputs, twice its 3 operand polynomials at width 1
    for batch, r, width in [(SIZE_MAX, 2, 1), (SIZE_MAX // 96 + 1, 3, 1), (SIZE_MAX // 48 + 1, 1, 3)]:
        assert _gram(lib, device, ctx, b, b, None, batch, r, r, width) == -1, (batch, r, width)
        msg = pkg._abi.last_error()
        assert "overflow" in msg and _name(device) + ":" in msg


@pytest.mark.parametrize("device", [False, True])
def test_empty_batch_is_a_no_op(pkg, fake, device):
    lib, b, ctx = fake
    # 0, whatever the checks that read the context would say: a family above the byte limit, g on top of a and b, a context of zeros
    for ra, rb, width in [(1, 1, 1), (3, 2, 5), (MAX_VECTORS, MAX_VECTORS, MAX_TERMS)]:
        assert _gram(lib, device, ctx, b, b, b, 0, ra, rb, width) == 0
        assert _gram(lib, device, ctx, b, b, None, 0, ra, ra, width) == 0
