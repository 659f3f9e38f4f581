"""CPU suite: the fold of ring vectors by ring-valued challenges (lsr_ntt_ring_fold_batch / _device) is declared, exported and mirrored
in ctypes, the Python methods exist on both context classes, and the argument checks that read no context run before any device work,
in batch.h's order — so they answer -1 with a message on a machine without a GPU, given a handle that is never dereferenced."""
import ctypes
import os
import re

import pytest

from ring_fold_model import test_gather_by_hand, test_schoolbook_fold_by_hand  # noqa: F401  (collected here: the model's own tests)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_H = os.path.join(ROOT, "include", "lambda_snark", "batch.h")
SYMBOLS = ["lsr_ntt_ring_fold_batch", "lsr_ntt_ring_fold_batch_device"]
SIZE_MAX = (1 << (8 * ctypes.sizeof(ctypes.c_size_t))) - 1


def _call(lib, device, ctx, out, v, p, outputs, terms, stride, width):
    if device:
        return lib.lsr_ntt_ring_fold_batch_device(ctx, out, v, p, outputs, terms, stride, width, None)
    return lib.lsr_ntt_ring_fold_batch(ctx, out, v, p, outputs, terms, stride, width)


@pytest.fixture()
def fake(pkg):
    """(library, a buffer address, the address of a context that is never dereferenced: the checks come first)"""
    buf = (ctypes.c_uint64 * 16)()
    ctx_buf = (ctypes.c_uint64 * 64)()
    yield pkg._abi.load_library(), ctypes.addressof(buf), ctypes.addressof(ctx_buf)
    del buf, ctx_buf


def test_batch_h_declares_the_fold():
    raw = open(BATCH_H).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
        assert m, name
        args = [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")]
        assert args[:8] == ["ctx", "out" if name == SYMBOLS[0] else "d_out", "v" if name == SYMBOLS[0] else "d_v", "p" if name == SYMBOLS[0] else "d_p",
                            "outputs", "terms", "term_stride", "width"], args
    assert re.search(r"#define\s+LSR_RING_FOLD_MAX_WIDTH\s+65536\b", text)


def test_library_exports_and_signatures(pkg):
    lib = pkg._abi.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in pkg._abi.SIGNATURES, name
    assert len(pkg._abi.SIGNATURES["lsr_ntt_ring_fold_batch"][1]) == 8
    assert len(pkg._abi.SIGNATURES["lsr_ntt_ring_fold_batch_device"][1]) == 9
    for cls in (pkg.NttContext, pkg.CyclicNtt):
        assert hasattr(cls, "ring_fold") and hasattr(cls, "ring_fold_device"), cls


def test_python_constant_mirrors_the_header(pkg):
    text = open(BATCH_H).read()
    assert int(re.search(r"#define\s+LSR_RING_FOLD_MAX_WIDTH\s+(\d+)", text).group(1)) == pkg.RING_FOLD_MAX_WIDTH == 65536


@pytest.mark.parametrize("device", [False, True])
def test_null_arguments_are_refused_first(pkg, fake, device):
    lib, b, fake_ctx = fake
    # (the later checks would fail too — terms = 0, width above the cap: NULL is reported first)
    for ctx, out, v, p in [(None, b, b, b), (fake_ctx, None, b, b), (fake_ctx, b, None, b), (fake_ctx, b, b, None)]:
        for outputs, terms, width in [(1, 1, 1), (3, 0, 1 << 20), (0, 1, 0)]:
            assert _call(lib, device, ctx, out, v, p, outputs, terms, 0, width) == -1
            msg = pkg._abi.last_error()
            assert "NULL" in msg and SYMBOLS[device] in msg


@pytest.mark.parametrize("device", [False, True])
def test_zero_terms_are_refused_before_the_empty_call(pkg, fake, device):
    lib, b, fake_ctx = fake
    for outputs, width in [(3, 2), (0, 2), (3, 0), (0, 0), (1, 1 << 20)]:      # an empty call is a no-op only after this check
        assert _call(lib, device, fake_ctx, b, b, b, outputs, 0, 0, width) == -1
        msg = pkg._abi.last_error()
        assert "terms" in msg and "width" not in msg


@pytest.mark.parametrize("device", [False, True])
def test_zero_outputs_or_width_is_a_no_op(pkg, fake, device):
    lib, b, fake_ctx = fake
    # as batch == 0 of the ring inner product: 0, whatever the later checks would say (terms and width above their caps)
    for outputs, terms, stride, width in [(0, 1, 0, 1), (0, 1 << 20, 5, 1 << 20), (4, 3, 3, 0), (0, 7, 0, 0), (SIZE_MAX, SIZE_MAX, SIZE_MAX, 0)]:
        assert _call(lib, device, fake_ctx, b, b, b, outputs, terms, stride, width) == 0


@pytest.mark.parametrize("device", [False, True])
def test_caps_are_refused_in_order(pkg, fake, device):
    lib, b, fake_ctx = fake
    too_many, too_wide = pkg.RING_DOT_MAX_TERMS + 1, pkg.RING_FOLD_MAX_WIDTH + 1
    assert _call(lib, device, fake_ctx, b, b, b, 1, too_many, 0, too_wide) == -1            # terms before width
    assert "LSR_RING_DOT_MAX_TERMS" in pkg._abi.last_error()
    assert _call(lib, device, fake_ctx, b, b, b, SIZE_MAX, 1, SIZE_MAX, too_wide) == -1      # width before the overflow
    assert "LSR_RING_FOLD_MAX_WIDTH" in pkg._abi.last_error()


@pytest.mark.parametrize("device", [False, True])
def test_overflowing_sizes_are_refused(pkg, fake, device):
    lib, b, fake_ctx = fake
    half = 1 << (4 * ctypes.sizeof(ctypes.c_size_t))          # half * half wraps to 0
    cases = [
        (half + 1, 1, half, 1),             # (outputs - 1) term_stride
        (2, 2, SIZE_MAX - 1, 1),            # ... + terms
        (2, 1, SIZE_MAX // 4, 8),           # vectors * width
        (SIZE_MAX // 2, 4, 0, 1),           # outputs * terms
        (SIZE_MAX // 2, 1, 0, 4),           # outputs * width
        (SIZE_MAX // 16 + 1, 1, 0, 1),      # bytes of the smallest ring
    ]
    for outputs, terms, stride, width in cases:
        assert _call(lib, device, fake_ctx, b, b, b, outputs, terms, stride, width) == -1, (outputs, terms, stride, width)
        msg = pkg._abi.last_error()
        assert "overflow" in msg and SYMBOLS[device] in msg
