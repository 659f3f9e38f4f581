"""CPU suite: the norms and projections of ring vectors (lsr_ntt_ring_l2sq_batch, lsr_ntt_ring_project_batch,
lsr_ntt_ring_project_matrix_batch and their _device forms) are declared, exported and mirrored in ctypes, the Python members exist on
both context classes, and the argument checks that read no context run before any device work, in batch.h's order — so they answer -1
with a message on a machine without a GPU, given a handle that is never dereferenced."""
import ctypes
import os
import re

import pytest

from ring_norm_model import (test_entry_map_by_hand,  # noqa: F401  (collected here: the model's own tests)
                             test_project_is_the_sum_over_its_own_matrix_rows,  # noqa: F401
                             test_projection_preserves_the_norm_for_the_fixed_seeds,  # noqa: F401
                             test_status_and_saturation_rules,  # noqa: F401
                             test_wrapping_sum_is_exact_at_the_accumulator_bound)  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_H = os.path.join(ROOT, "include", "lambda_snark", "batch.h")
L2, PROJECT, MATRIX = "lsr_ntt_ring_l2sq_batch", "lsr_ntt_ring_project_batch", "lsr_ntt_ring_project_matrix_batch"
ARGUMENTS = {
    L2: ["ctx", "x", "count", "width", "out"],
    L2 + "_device": ["ctx", "d_x", "count", "width", "d_out", "stream"],
    PROJECT: ["ctx", "out", "status", "x", "count", "width", "bound", "keys", "components", "domain", "index_base"],
    PROJECT + "_device": ["ctx", "d_out", "d_status", "d_x", "count", "width", "bound", "d_keys", "components", "domain", "index_base", "stream"],
    MATRIX: ["ctx", "out", "rows_first", "rows", "width", "key", "domain", "index_base"],
    MATRIX + "_device": ["ctx", "d_out", "rows_first", "rows", "width", "d_key", "domain", "index_base", "stream"],
}
SIZE_MAX = (1 << (8 * ctypes.sizeof(ctypes.c_size_t))) - 1
HALF = 1 << (4 * ctypes.sizeof(ctypes.c_size_t))          # HALF * HALF wraps to 0


def _name(base, device):
    return base + "_device" if device else base


def _l2(lib, device, ctx, x, count, width, out):
    if device:
        return lib.lsr_ntt_ring_l2sq_batch_device(ctx, x, count, width, out, None)
    return lib.lsr_ntt_ring_l2sq_batch(ctx, x, count, width, out)


def _project(lib, device, ctx, out, status, x, count, width, bound, keys, components, domain=17, index_base=0):
    if device:
        return lib.lsr_ntt_ring_project_batch_device(ctx, out, status, x, count, width, bound, keys, components, domain, index_base, None)
    return lib.lsr_ntt_ring_project_batch(ctx, out, status, x, count, width, bound, keys, components, domain, index_base)


def _matrix(lib, device, ctx, out, rows_first, rows, width, key, domain=17, index_base=0):
    if device:
        return lib.lsr_ntt_ring_project_matrix_batch_device(ctx, out, rows_first, rows, width, key, domain, index_base, None)
    return lib.lsr_ntt_ring_project_matrix_batch(ctx, out, rows_first, rows, width, key, domain, index_base)


@pytest.fixture()
def fake(pkg):
    """(library, a buffer address, the address of a context that is never dereferenced: the checks come first)"""
    buf = (ctypes.c_uint64 * 16)()
    ctx_buf = (ctypes.c_uint64 * 64)()
    yield pkg._abi.load_library(), ctypes.addressof(buf), ctypes.addressof(ctx_buf)
    del buf, ctx_buf


def test_batch_h_declares_the_six_functions_and_offers_the_l2_norm():
    raw = open(BATCH_H).read()
    assert "not offered" not in raw
    assert re.search(r"#define\s+LSR_RING_PROJECT_ROWS\s+256\b", raw)
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
    assert [len(pkg._abi.SIGNATURES[name][1]) for name in ARGUMENTS] == [5, 6, 11, 12, 8, 9]
    assert pkg.RING_PROJECT_ROWS == 256
    for cls in (pkg.NttContext, pkg.CyclicNtt):
        for member in ("ring_l2sq", "ring_l2sq_device", "ring_project", "ring_project_device", "ring_project_matrix", "ring_project_matrix_device"):
            assert callable(getattr(cls, member)), (cls, member)


@pytest.mark.parametrize("device", [False, True])
def test_null_arguments_are_refused_first(pkg, fake, device):
    lib, b, ctx = fake
    # (the later checks would fail too — no components, no bound, rows past 256, overflowing sizes: NULL is reported first)
    for args in [(None, b, b), (ctx, None, b), (ctx, b, None)]:
        for count, width in [(1, 1), (0, 0), (SIZE_MAX, SIZE_MAX)]:
            assert _l2(lib, device, args[0], args[1], count, width, args[2]) == -1
            msg = pkg._abi.last_error()
            assert "NULL" in msg and _name(L2, device) + ":" in msg
    for hole in range(5):
        c, out, status, x, keys = [None if i == hole else (ctx if i == 0 else b) for i in range(5)]
        for count, width, bound, components in [(1, 1, 1, 1), (0, 0, 0, 0), (SIZE_MAX, SIZE_MAX, 0, 0)]:
            assert _project(lib, device, c, out, status, x, count, width, bound, keys, components) == -1
            msg = pkg._abi.last_error()
            assert "NULL" in msg and _name(PROJECT, device) + ":" in msg
    for hole in range(3):
        c, out, key = [None if i == hole else (ctx if i == 0 else b) for i in range(3)]
        for rows_first, rows, width in [(0, 1, 1), (200, 100, 0), (SIZE_MAX, SIZE_MAX, SIZE_MAX)]:
            assert _matrix(lib, device, c, out, rows_first, rows, width, key) == -1
            msg = pkg._abi.last_error()
            assert "NULL" in msg and _name(MATRIX, device) + ":" in msg


@pytest.mark.parametrize("device", [False, True])
def test_components_bound_and_rows_are_refused_before_the_empty_call(pkg, fake, device):
    lib, b, ctx = fake
    for count, width in [(0, 0), (0, 3), (3, 0), (2, 2), (SIZE_MAX, SIZE_MAX)]:
        for bound in [0, 1]:                                   # components before bound
            assert _project(lib, device, ctx, b, b, b, count, width, bound, b, 0) == -1
            msg = pkg._abi.last_error()
            assert "components" in msg and "bound" not in msg and _name(PROJECT, device) + ":" in msg
        assert _project(lib, device, ctx, b, b, b, count, width, 0, b, 1) == -1
        msg = pkg._abi.last_error()
        assert "bound" in msg and "components" not in msg and _name(PROJECT, device) + ":" in msg
    for rows_first, rows in [(0, 257), (1, 256), (256, 1), (257, 0), (SIZE_MAX, 2), (2, SIZE_MAX), (SIZE_MAX, SIZE_MAX)]:
        for width in [0, 1, SIZE_MAX]:
            assert _matrix(lib, device, ctx, b, rows_first, rows, width, b) == -1, (rows_first, rows)
            msg = pkg._abi.last_error()
            assert "256" in msg and "rows_first" in msg and _name(MATRIX, device) + ":" in msg


@pytest.mark.parametrize("device", [False, True])
def test_empty_calls_are_no_ops(pkg, fake, device):
    lib, b, ctx = fake
    # 0, whatever the later checks would say: products that overflow, a bound above every q, an index that wraps
    for count, width in [(0, 0), (0, 1), (1, 0), (0, SIZE_MAX), (SIZE_MAX, 0)]:
        assert _l2(lib, device, ctx, b, count, width, b) == 0
        assert _project(lib, device, ctx, b, b, b, count, width, (1 << 64) - 1, b, SIZE_MAX, 17, (1 << 64) - 1) == 0
    for rows_first, rows, width in [(0, 0, 1), (256, 0, 1), (0, 256, 0), (3, 0, SIZE_MAX), (0, 1, 0)]:
        assert _matrix(lib, device, ctx, b, rows_first, rows, width, b, 17, (1 << 64) - 1) == 0


@pytest.mark.parametrize("device", [False, True])
def test_overflowing_sizes_are_refused(pkg, fake, device):
    lib, b, ctx = fake
    # count * width; that times 16 bytes (the smallest ring); count * 256 * 8
    for count, width in [(HALF, HALF), (SIZE_MAX, 2), (SIZE_MAX // 16 + 1, 1), (1, SIZE_MAX // 16 + 1), (SIZE_MAX // 64 + 1, 4)]:
        assert _l2(lib, device, ctx, b, count, width, b) == -1, (count, width)
        msg = pkg._abi.last_error()
        assert "overflow" in msg and _name(L2, device) + ":" in msg
        assert _project(lib, device, ctx, b, b, b, count, width, 1, b, 1) == -1, (count, width)
        msg = pkg._abi.last_error()
        assert "overflow" in msg and _name(PROJECT, device) + ":" in msg
    assert SIZE_MAX // 2048 + 1 <= SIZE_MAX // 16                # count * 1 * 16 fits, count * 256 * 8 does not
    assert _project(lib, device, ctx, b, b, b, SIZE_MAX // 2048 + 1, 1, 1, b, 1) == -1
    msg = pkg._abi.last_error()
    assert "overflow" in msg and _name(PROJECT, device) + ":" in msg
    for rows, width in [(256, SIZE_MAX // 256 + 1), (1, SIZE_MAX // 16 + 1), (2, SIZE_MAX // 32 + 1)]:
        assert _matrix(lib, device, ctx, b, 0, rows, width, b) == -1, (rows, width)
        msg = pkg._abi.last_error()
        assert "overflow" in msg and _name(MATRIX, device) + ":" in msg
