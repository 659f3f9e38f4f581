"""CPU suite: the ring matrix-vector product with a resident matrix (LsrRingMatrix, lsr_ntt_ring_matrix_* and
lsr_ntt_ring_matvec_batch / _device) is declared, exported and mirrored in ctypes, and its argument checks run before any device
work, in the documented order — so they answer NULL / -1 with a message on a machine without a GPU."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_H = os.path.join(ROOT, "include", "lambda_snark", "batch.h")
SYMBOLS = {
    "lsr_ntt_ring_matrix_create": r"LsrRingMatrix\s*\*", "lsr_ntt_ring_matrix_create_device": r"LsrRingMatrix\s*\*",
    "lsr_ntt_ring_matrix_free": r"void", "lsr_ntt_ring_matrix_rows": r"size_t", "lsr_ntt_ring_matrix_cols": r"size_t",
    "lsr_ntt_ring_matrix_row_block": r"size_t", "lsr_ntt_ring_matvec_batch": r"int", "lsr_ntt_ring_matvec_batch_device": r"int",
}
CAPS = {"LSR_RING_MATVEC_MAX_ROWS": "RING_MATVEC_MAX_ROWS", "LSR_RING_MATVEC_MAX_MATRIX_BYTES": "RING_MATVEC_MAX_MATRIX_BYTES",
        "LSR_RING_DOT_MAX_TERMS": "RING_DOT_MAX_TERMS"}


def _create(lib, device, ctx, m, rows, cols):
    if device:
        return lib.lsr_ntt_ring_matrix_create_device(ctx, m, rows, cols, None)
    return lib.lsr_ntt_ring_matrix_create(ctx, m, rows, cols)


def _matvec(lib, device, mat, y, x, batch):
    if device:
        return lib.lsr_ntt_ring_matvec_batch_device(mat, y, x, batch, None)
    return lib.lsr_ntt_ring_matvec_batch(mat, y, x, batch)


@pytest.fixture()
def fake(pkg):
    """(library, a buffer address, the address of a context / matrix handle that is never dereferenced: the checks come first)"""
    buf = (ctypes.c_uint64 * 16)()
    handle_buf = (ctypes.c_uint64 * 64)()
    yield pkg._abi.load_library(), ctypes.addressof(buf), ctypes.addressof(handle_buf)
    del buf, handle_buf


def test_batch_h_declares_the_matrix_and_the_product():
    raw = open(BATCH_H).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"typedef\s+struct\s+LsrRingMatrix\s+LsrRingMatrix\s*;", text)
    for name, ret in SYMBOLS.items():
        assert re.search(ret + r"\s*" + name + r"\s*\(", text), name
    for cap in CAPS:
        assert re.search(r"#define\s+" + cap + r"\s+\d+", text), cap
    assert text.index("lsr_ntt_ring_dot_batch_device") < text.index("LsrRingMatrix") < text.index("lsr_sample_gaussian_seeded")
    assert "outlive" in raw                                # the lifetime rule of the handle is stated


def test_library_exports_and_signatures(pkg):
    lib = pkg._abi.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in pkg._abi.SIGNATURES, name
    counts = {"lsr_ntt_ring_matrix_create": 4, "lsr_ntt_ring_matrix_create_device": 5, "lsr_ntt_ring_matrix_free": 1,
              "lsr_ntt_ring_matrix_rows": 1, "lsr_ntt_ring_matrix_cols": 1, "lsr_ntt_ring_matrix_row_block": 1,
              "lsr_ntt_ring_matvec_batch": 4, "lsr_ntt_ring_matvec_batch_device": 5}
    for name, count in counts.items():
        assert len(pkg._abi.SIGNATURES[name][1]) == count, name
    for cls in (pkg.NttContext, pkg.CyclicNtt):
        assert hasattr(cls, "ring_matrix") and hasattr(cls, "ring_matrix_device")
    for attr in ("rows", "cols", "row_block", "matvec", "matvec_device", "close"):
        assert hasattr(pkg.RingMatrix, attr), attr


def test_python_constants_mirror_the_header(pkg):
    text = open(BATCH_H).read()
    for cap, mirror in CAPS.items():
        assert int(re.search(r"#define\s+" + cap + r"\s+(\d+)", text).group(1)) == getattr(pkg, mirror), cap
    assert pkg.RING_MATVEC_MAX_MATRIX_BYTES >= 64 * 256 * 4096 * 8       # the 64 x 256 matrix at n = 4096
    # the y words of one tile (4096 * rows) and its x words (4096 * cols) stay within a 2^31-byte buffer range
    assert pkg.RING_MATVEC_MAX_ROWS * 4096 * 8 < 2**31 and pkg.RING_DOT_MAX_TERMS * 4096 * 8 <= 2**31


@pytest.mark.parametrize("device", [False, True])
def test_create_refuses_null_arguments(pkg, fake, device):
    lib, p, fake_ctx = fake
    # (rows = 0 would fail too: NULL is reported first)
    for ctx, m in [(None, p), (fake_ctx, None)]:
        for rows, cols in [(1, 1), (0, 3)]:
            assert not _create(lib, device, ctx, m, rows, cols)
            msg = pkg._abi.last_error()
            assert msg and "NULL" in msg


@pytest.mark.parametrize("device", [False, True])
def test_create_refuses_zero_and_over_cap_sizes_naming_the_argument(pkg, fake, device):
    lib, p, fake_ctx = fake
    big_rows, big_cols = pkg.RING_MATVEC_MAX_ROWS + 1, pkg.RING_DOT_MAX_TERMS + 1
    cases = [(0, 3, "rows"), (3, 0, "cols"), (0, 0, "rows"), (big_rows, 1, "rows"), (1, big_cols, "cols"), (0, big_cols, "rows"),
             (big_rows, 0, "cols")]
    for rows, cols, named in cases:
        assert not _create(lib, device, fake_ctx, p, rows, cols), (rows, cols)
        msg = pkg._abi.last_error()
        other = "cols" if named == "rows" else "rows"
        assert named in msg and other not in msg, (rows, cols, msg)
    assert "LSR_RING_MATVEC_MAX_ROWS" in (_create(lib, device, fake_ctx, p, big_rows, 1) or pkg._abi.last_error())
    assert "LSR_RING_DOT_MAX_TERMS" in (_create(lib, device, fake_ctx, p, 1, big_cols) or pkg._abi.last_error())
    # within both caps, but too many polynomials for the byte cap at any n (n >= 2)
    rows, cols = pkg.RING_MATVEC_MAX_ROWS, pkg.RING_MATVEC_MAX_MATRIX_BYTES // 16 // pkg.RING_MATVEC_MAX_ROWS + 1
    assert cols <= pkg.RING_DOT_MAX_TERMS
    assert not _create(lib, device, fake_ctx, p, rows, cols)
    assert "LSR_RING_MATVEC_MAX_MATRIX_BYTES" in pkg._abi.last_error()


def test_null_handle_accessors(pkg):
    lib = pkg._abi.load_library()
    lib.lsr_ntt_ring_matrix_free(None)
    assert lib.lsr_ntt_ring_matrix_rows(None) == 0
    assert lib.lsr_ntt_ring_matrix_cols(None) == 0
    assert lib.lsr_ntt_ring_matrix_row_block(None) == 0


@pytest.mark.parametrize("device", [False, True])
def test_matvec_refuses_null_arguments(pkg, fake, device):
    lib, p, fake_mat = fake
    for mat, y, x in [(None, p, p), (fake_mat, None, p), (fake_mat, p, None)]:
        for batch in (1, 0):                                 # NULL is reported before the batch == 0 no-op
            assert _matvec(lib, device, mat, y, x, batch) == -1
            msg = pkg._abi.last_error()
            assert msg and "NULL" in msg


@pytest.mark.parametrize("device", [False, True])
def test_empty_batch_is_a_no_op(pkg, fake, device):
    lib, p, fake_mat = fake
    assert _matvec(lib, device, fake_mat, p, p, 0) == 0
    assert _matvec(lib, device, fake_mat, p, p + 8, 0) == 0
