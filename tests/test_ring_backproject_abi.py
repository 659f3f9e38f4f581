"""CPU suite: the adjoint of the seeded projection (lsr_ntt_ring_project_adjoint_batch and its _device form) is
declared, exported and mirrored in ctypes, the Python members exist on both context classes, and the argument checks that read no
context run before any device work, in batch.h's order — so they answer -1 with a message on a machine without a GPU, given a handle
that is never dereferenced."""
import ctypes
import os
import re

import pytest

from ring_backproject_model import (test_adjoint_identity_against_the_projection,  # noqa: F401  (collected here: the model's own tests)
                                    test_all_weights_q_minus_1_at_the_widest_moduli,  # noqa: F401
                                    test_status_rule,  # noqa: F401
                                    test_unit_weight_gives_the_matrix_row,  # noqa: F401
                                    test_weighted_columns_by_hand_on_one_stream_word)  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_H = os.path.join(ROOT, "include", "lambda_snark", "batch.h")
ADJOINT = "lsr_ntt_ring_project_adjoint_batch"
ARGUMENTS = {
    ADJOINT: ["ctx", "out", "status", "weights", "count", "sets", "width", "conjugate", "keys", "components", "domain", "index_base"],
    ADJOINT + "_device": ["ctx", "d_out", "d_status", "d_weights", "count", "sets", "width", "conjugate", "d_keys", "components", "domain",
                          "index_base", "stream"],
}
SIZE_MAX = (1 << (8 * ctypes.sizeof(ctypes.c_size_t))) - 1
HALF = 1 << (4 * ctypes.sizeof(ctypes.c_size_t))          # HALF * HALF wraps to 0


def _name(device):
    return ADJOINT + "_device" if device else ADJOINT


def _adjoint(lib, device, ctx, out, status, weights, count, sets, width, conjugate, keys, components, domain=17, index_base=0):
    if device:
        return lib.lsr_ntt_ring_project_adjoint_batch_device(ctx, out, status, weights, count, sets, width, conjugate, keys, components, domain,
                                                             index_base, None)
    return lib.lsr_ntt_ring_project_adjoint_batch(ctx, out, status, weights, count, sets, width, conjugate, keys, components, domain, index_base)


@pytest.fixture()
def fake(pkg):
    """(library, a buffer address, the address of a context that is never dereferenced: the checks come first)"""
    buf = (ctypes.c_uint64 * 16)()
    ctx_buf = (ctypes.c_uint64 * 64)()
    yield pkg._abi.load_library(), ctypes.addressof(buf), ctypes.addressof(ctx_buf)
    del buf, ctx_buf


def test_batch_h_declares_the_two_functions_and_the_macro():
    raw = open(BATCH_H).read()
    assert re.search(r"#define\s+LSR_RING_PROJECT_ADJOINT_MAX_SETS\s+16\b", raw)
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
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
    assert [len(pkg._abi.SIGNATURES[name][1]) for name in ARGUMENTS] == [12, 13]
    assert pkg.RING_PROJECT_ADJOINT_MAX_SETS == 16 and "RING_PROJECT_ADJOINT_MAX_SETS" in pkg.__all__
    for cls in (pkg.NttContext, pkg.CyclicNtt):
        for member in ("ring_project_adjoint", "ring_project_adjoint_device"):
            assert callable(getattr(cls, member)), (cls, member)


@pytest.mark.parametrize("device", [False, True])
def test_null_arguments_are_refused_first(pkg, fake, device):
    lib, b, ctx = fake
    # (the later checks would fail too — no components, no sets, a conjugate of 2, overflowing sizes: NULL is reported first)
    for hole in range(5):
        c, out, status, weights, keys = [None if i == hole else (ctx if i == 0 else b) for i in range(5)]
        for count, sets, width, conjugate, components in [(1, 1, 1, 0, 1), (0, 0, 0, 2, 0), (SIZE_MAX, 17, SIZE_MAX, -1, 0)]:
            assert _adjoint(lib, device, c, out, status, weights, count, sets, width, conjugate, keys, components) == -1
            msg = pkg._abi.last_error()
            assert "NULL" in msg and _name(device) + ":" in msg


@pytest.mark.parametrize("device", [False, True])
def test_components_sets_and_conjugate_are_refused_in_that_order_before_the_empty_call(pkg, fake, device):
    lib, b, ctx = fake
    for count, width in [(0, 0), (0, 3), (3, 0), (2, 2), (SIZE_MAX, SIZE_MAX)]:
        for sets, conjugate in [(0, 0), (17, 2), (1, 0)]:        # components before sets and conjugate
            assert _adjoint(lib, device, ctx, b, b, b, count, sets, width, conjugate, b, 0) == -1
            msg = pkg._abi.last_error()
            assert "components" in msg and "sets" not in msg and "conjugate" not in msg and _name(device) + ":" in msg
        for sets in [0, 17, SIZE_MAX]:                            # sets before conjugate
            for conjugate in [0, 2]:
                assert _adjoint(lib, device, ctx, b, b, b, count, sets, width, conjugate, b, 1) == -1
                msg = pkg._abi.last_error()
                assert "sets" in msg and "16" in msg and "conjugate" not in msg and _name(device) + ":" in msg
        for conjugate in [2, -1, 256]:
            for sets in [1, 16]:
                assert _adjoint(lib, device, ctx, b, b, b, count, sets, width, conjugate, b, 1) == -1
                msg = pkg._abi.last_error()
                assert "conjugate" in msg and _name(device) + ":" in msg


@pytest.mark.parametrize("device", [False, True])
def test_empty_calls_are_no_ops(pkg, fake, device):
    lib, b, ctx = fake
    # 0, whatever the later checks would say: products that overflow, an index that wraps
    for count, width in [(0, 0), (0, 1), (1, 0), (0, SIZE_MAX), (SIZE_MAX, 0)]:
        for sets, conjugate in [(1, 0), (16, 1)]:
            assert _adjoint(lib, device, ctx, b, b, b, count, sets, width, conjugate, b, SIZE_MAX, 17, (1 << 64) - 1) == 0


@pytest.mark.parametrize("device", [False, True])
def test_overflowing_sizes_are_refused(pkg, fake, device):
    lib, b, ctx = fake
    # count * sets; that times width; that times 16 bytes (the smallest ring)
    cases = [(SIZE_MAX // 16 + 1, 16, 1), (SIZE_MAX // 2, 3, 1), (HALF, 1, HALF), (HALF // 16, 16, HALF), (SIZE_MAX, 1, 2),
             (SIZE_MAX // 16 + 1, 1, 1), (1, 1, SIZE_MAX // 16 + 1), (SIZE_MAX // 64 + 1, 2, 2), (1, 16, SIZE_MAX // 256 + 1)]
    for count, sets, width in cases:
        for conjugate in [0, 1]:
            assert _adjoint(lib, device, ctx, b, b, b, count, sets, width, conjugate, b, 1) == -1, (count, sets, width)
            msg = pkg._abi.last_error()
            assert "overflow" in msg and _name(device) + ":" in msg
