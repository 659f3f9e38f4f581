"""CPU suite: the scalar-weighted aggregation of ring vectors (lsr_ntt_ring_scalar_combine_batch and its _device form)
is declared, exported and mirrored in ctypes, the Python members exist on both context classes, and the argument checks that read no
context run before any device work, in batch.h's order — so they answer -1 with a message on a machine without a GPU, given a handle
that is never dereferenced."""
import ctypes
import os
import re

import pytest

from ring_scalar_model import (test_all_words_q_minus_1,  # noqa: F401  (collected here: the model's own tests)
                               test_status_rule,  # noqa: F401
                               test_two_by_two_by_hand,  # noqa: F401
                               test_unit_weight_returns_the_term_plus_the_addend)  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_H = os.path.join(ROOT, "include", "lambda_snark", "batch.h")
COMBINE = "lsr_ntt_ring_scalar_combine_batch"
ARGUMENTS = {
    COMBINE: ["ctx", "out", "status", "v", "weights", "addend", "count", "sets", "terms", "term_stride", "width", "components"],
    COMBINE + "_device": ["ctx", "d_out", "d_status", "d_v", "d_weights", "d_addend", "count", "sets", "terms", "term_stride", "width", "components",
                          "stream"],
}
SIZE_MAX = (1 << (8 * ctypes.sizeof(ctypes.c_size_t))) - 1
HALF = 1 << (4 * ctypes.sizeof(ctypes.c_size_t))          # HALF * HALF wraps to 0
MAX_TERMS = 65536


def _name(device):
    return COMBINE + "_device" if device else COMBINE


def _combine(lib, device, ctx, out, status, v, weights, addend, count, sets, terms, term_stride, width, components):
    if device:
        return lib.lsr_ntt_ring_scalar_combine_batch_device(ctx, out, status, v, weights, addend, count, sets, terms, term_stride, width, components, None)
    return lib.lsr_ntt_ring_scalar_combine_batch(ctx, out, status, v, weights, addend, count, sets, terms, term_stride, width, components)


@pytest.fixture()
def fake(pkg):
    """(library, a buffer address, the address of a context that is never dereferenced: the checks come first)"""
    buf = (ctypes.c_uint64 * 16)()
    ctx_buf = (ctypes.c_uint64 * 64)()
    yield pkg._abi.load_library(), ctypes.addressof(buf), ctypes.addressof(ctx_buf)
    del buf, ctx_buf


def test_batch_h_declares_the_two_functions_and_the_macros():
    raw = open(BATCH_H).read()
    assert re.search(r"#define\s+LSR_RING_SCALAR_COMBINE_MAX_SETS\s+16\b", raw)
    assert re.search(r"#define\s+LSR_RING_SCALAR_COMBINE_TILE\s+\d+\b", raw) and re.search(r"#define\s+LSR_RING_SCALAR_COMBINE_STAGE\s+\d+\b", raw)
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, want in ARGUMENTS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
        assert m, name
        assert [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")] == want, name
    assert text.index(COMBINE) > text.index("lsr_ntt_ring_project_adjoint_batch_device")      # behind the adjoint's block


def test_library_exports_signatures_and_members(pkg):
    lib = pkg._abi.load_library()
    for name, want in ARGUMENTS.items():
        assert hasattr(lib, name), name
        assert name in pkg._abi.SIGNATURES, name
        assert len(pkg._abi.SIGNATURES[name][1]) == len(want), name
    assert [len(pkg._abi.SIGNATURES[name][1]) for name in ARGUMENTS] == [12, 13]
    assert pkg.RING_SCALAR_COMBINE_MAX_SETS == 16 and "RING_SCALAR_COMBINE_MAX_SETS" in pkg.__all__
    assert pkg.RING_DOT_MAX_TERMS == MAX_TERMS
    for cls in (pkg.NttContext, pkg.CyclicNtt):
        for member in ("ring_scalar_combine", "ring_scalar_combine_device"):
            assert callable(getattr(cls, member)), (cls, member)


@pytest.mark.parametrize("device", [False, True])
def test_null_arguments_are_refused_first(pkg, fake, device):
    lib, b, ctx = fake
    # (the later checks would fail too — no components, no sets, no terms, overflowing sizes: NULL is reported first)
    for hole in range(5):
        c, out, status, v, weights = [None if i == hole else (ctx if i == 0 else b) for i in range(5)]
        for addend in (None, b):
            for count, sets, terms, ts, width, components in [(1, 1, 1, 0, 1, 1), (0, 0, 0, 0, 0, 0), (SIZE_MAX, 17, MAX_TERMS + 1, SIZE_MAX, SIZE_MAX, 0)]:
                assert _combine(lib, device, c, out, status, v, weights, addend, count, sets, terms, ts, width, components) == -1
                msg = pkg._abi.last_error()
                assert "NULL" in msg and _name(device) + ":" in msg
    # a NULL addend is not an error: the call goes on to the next check
    assert _combine(lib, device, ctx, b, b, b, b, None, 1, 1, 1, 0, 1, 0) == -1 and "components" in pkg._abi.last_error()


@pytest.mark.parametrize("device", [False, True])
def test_components_sets_and_terms_are_refused_in_that_order_before_the_empty_call(pkg, fake, device):
    lib, b, ctx = fake
    for count, width in [(0, 0), (0, 3), (3, 0), (2, 2), (SIZE_MAX, SIZE_MAX)]:
        for sets, terms in [(0, 0), (17, MAX_TERMS + 1), (1, 1)]:            # components before sets and terms
            assert _combine(lib, device, ctx, b, b, b, b, None, count, sets, terms, 0, width, 0) == -1
            msg = pkg._abi.last_error()
            assert "components" in msg and "sets" not in msg and "terms" not in msg and _name(device) + ":" in msg
        for sets in [0, 17, SIZE_MAX]:                                        # sets before terms
            for terms in [0, 1, MAX_TERMS + 1]:
                assert _combine(lib, device, ctx, b, b, b, b, None, count, sets, terms, 0, width, 1) == -1
                msg = pkg._abi.last_error()
                assert "sets" in msg and "16" in msg and "terms" not in msg and _name(device) + ":" in msg
        for terms in [0, MAX_TERMS + 1, SIZE_MAX]:
            for sets in [1, 16]:
                assert _combine(lib, device, ctx, b, b, b, b, None, count, sets, terms, 0, width, 1) == -1
                msg = pkg._abi.last_error()
                assert "terms" in msg and "LSR_RING_DOT_MAX_TERMS" in msg and "overflow" not in msg and _name(device) + ":" in msg


@pytest.mark.parametrize("device", [False, True])
def test_empty_calls_are_no_ops(pkg, fake, device):
    lib, b, ctx = fake
    # 0, whatever the later checks would say: products that overflow
    for count, width in [(0, 0), (0, 1), (1, 0), (0, SIZE_MAX), (SIZE_MAX, 0)]:
        for sets, terms, ts in [(1, 1, 0), (16, MAX_TERMS, SIZE_MAX)]:
            for addend in (None, b):
                assert _combine(lib, device, ctx, b, b, b, b, addend, count, sets, terms, ts, width, SIZE_MAX) == 0


@pytest.mark.parametrize("device", [False, True])
def test_overflowing_sizes_are_refused(pkg, fake, device):
    lib, b, ctx = fake
    # (count, sets, terms, term_stride, width, components)
    cases = [(3, 1, 1, SIZE_MAX // 2 + 1, 1, 1),               # (count - 1) term_stride
             (2, 1, 2, SIZE_MAX - 1, 1, 1),                    # ... + terms
             (HALF + 1, 1, 1, 1, HALF, 1),                     # vectors * width
             (1, 1, MAX_TERMS, 0, SIZE_MAX // MAX_TERMS + 1, 1),
             (SIZE_MAX // 16 + 1, 16, 1, 0, 1, SIZE_MAX),      # count * sets
             (SIZE_MAX // 2, 3, 1, 0, 1, SIZE_MAX),
             (HALF // 16, 16, 1, 0, HALF, SIZE_MAX),           # count * sets * width
             (1, 16, 1, 0, SIZE_MAX // 16 + 1, 1),
             (SIZE_MAX // 4 + 1, 1, 4, 0, 1, 1),               # groups * sets * terms (term_stride 0: v stays small)
             (SIZE_MAX // 16 + 1, 1, 1, 0, 1, SIZE_MAX),       # count * sets * 16 bytes
             (1, 1, 1, 0, SIZE_MAX // 16 + 1, 1),              # vectors * width * 16 bytes
             (SIZE_MAX // 64 + 1, 2, 2, 0, 2, 1)]              # groups * sets * terms * 16 bytes
    for count, sets, terms, ts, width, components in cases:
        for addend in (None, b):
            assert _combine(lib, device, ctx, b, b, b, b, addend, count, sets, terms, ts, width, components) == -1, (count, sets, terms, ts, width)
            msg = pkg._abi.last_error()
            assert "overflow" in msg and _name(device) + ":" in msg
