"""CPU suite: the seeded ring sampling calls (lsr_ring_sample_key_from_seed, lsr_ntt_ring_sample_batch(_device),
lsr_ntt_ring_matrix_create_seeded) are declared, exported and mirrored in ctypes; the host-only key expansion is the documented one;
and the refusals that read no context (NULL, then the kind and components == 0; for the seeded matrix the shape rules of
lsr_ntt_ring_matrix_create) come first, in the documented order — checked with fake handles that are never dereferenced.  The refusals
behind them read q and n of the context and are checked on the GPU (test_ring_sample_gpu.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

import ring_sample_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_H = os.path.join(ROOT, "include", "lambda_snark", "batch.h")
# name -> (return type, number of arguments)
SYMBOLS = {
    "lsr_ring_sample_key_from_seed": (r"void", 2),
    "lsr_ntt_ring_sample_batch": (r"int", 9), "lsr_ntt_ring_sample_batch_device": (r"int", 10),
    "lsr_ntt_ring_matrix_create_seeded": (r"LsrRingMatrix\s*\*", 6),
}
CONSTANTS = {"LSR_RING_SAMPLE_UNIFORM": "RING_SAMPLE_UNIFORM", "LSR_RING_SAMPLE_BOUNDED": "RING_SAMPLE_BOUNDED",
             "LSR_RING_SAMPLE_BALL": "RING_SAMPLE_BALL", "LSR_RING_SAMPLE_MAX_WORDS": "RING_SAMPLE_MAX_WORDS"}


@pytest.fixture()
def fake(pkg):
    """(library, a buffer address, the address of a context that is never dereferenced: the checks under test come first)"""
    buf = (ctypes.c_uint64 * 16)()
    handle_buf = (ctypes.c_uint64 * 64)()
    yield pkg._abi.load_library(), ctypes.addressof(buf), ctypes.addressof(handle_buf)
    del buf, handle_buf


def _sample(lib, device, ctx, out, count, kind, param, keys, components, domain=16, index_base=0):
    if device:
        return lib.lsr_ntt_ring_sample_batch_device(ctx, out, count, kind, param, keys, components, domain, index_base, None)
    return lib.lsr_ntt_ring_sample_batch(ctx, out, count, kind, param, keys, components, domain, index_base)


def _name(device):
    return "lsr_ntt_ring_sample_batch_device" if device else "lsr_ntt_ring_sample_batch"


def test_batch_h_declares_the_block_with_its_definitions():
    raw = open(BATCH_H).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, (ret, count) in SYMBOLS.items():
        found = re.search(ret + r"\s*" + name + r"\s*\(([^)]*)\)", text)
        assert found, name
        assert len(found.group(1).split(",")) == count, name
    assert text.index("lsr_ntt_ring_matvec_gadget_batch_device") < text.index("lsr_ring_sample_key_from_seed") < text.index("lsr_sample_gaussian_seeded")
    for word in ("draw(m; w_0, w_1, ...; U)", "L = bitlen(m - 1)", "F = floor(U / L)", "keys[4 (e / components) ..]", "index_base + (e % components)",
                 "c[i] = c[j]", "U = 63", "NOT constant-time", "below 2^28", "SHA3 digest"):
        assert word in raw, word                                # the definitions are the contract and live in the header


def test_library_exports_signatures_wrappers_and_constants(pkg):
    lib = pkg._abi.load_library()
    for name, (_, count) in SYMBOLS.items():
        assert hasattr(lib, name), name
        assert len(pkg._abi.SIGNATURES[name][1]) == count, name
    for cls in (pkg.NttContext, pkg.CyclicNtt):
        for attr in ("ring_sample", "ring_sample_device", "ring_matrix_seeded"):
            assert hasattr(cls, attr), (cls, attr)
    text = open(BATCH_H).read()
    for macro, mirror in CONSTANTS.items():
        assert int(re.search(r"#define\s+" + macro + r"\s+(\d+)", text).group(1)) == getattr(pkg, mirror), macro
        assert mirror in pkg.__all__
    assert (pkg.RING_SAMPLE_UNIFORM, pkg.RING_SAMPLE_BOUNDED, pkg.RING_SAMPLE_BALL) == (model.UNIFORM, model.BOUNDED, model.BALL)
    assert pkg.RING_SAMPLE_MAX_WORDS == model.MAX_WORDS == 64 and "ring_sample_key" in pkg.__all__


def test_key_from_seed_is_the_documented_expansion(pkg):
    lib = pkg._abi.load_library()
    for seed in (0, 1, 135, 0x0123456789ABCDEF, 2**64 - 1):
        key = pkg.ring_sample_key(seed)
        assert key.dtype == np.uint64 and [int(w) for w in key] == model.key_from_seed(seed)
        words32 = key.view("<u4")
        assert [int(w) for w in words32] == [seed & 0xFFFFFFFF, seed >> 32, int.from_bytes(b"LSR1", "little"), int.from_bytes(b"STRM", "little"), 0, 0, 0, 0]
    lib.lsr_ring_sample_key_from_seed(5, None)                  # NULL-safe


def test_key_from_seed_keys_the_oracle_stream(pkg, oracle):
    """The expansion is the one the oracle's stream_words applies: block 0 under the key, read as a full 256-bit key, is words 0..7."""
    key = pkg.ring_sample_key(99)
    block = oracle.chacha20_block(key.view("<u4"), 0, [16, 3, 0])
    words = [int(block[2 * j]) | (int(block[2 * j + 1]) << 32) for j in range(8)]
    assert words == [int(w) for w in oracle.stream_words(99, 16, 3, 0, 8)]


@pytest.mark.parametrize("device", [False, True])
def test_null_is_refused_first(pkg, fake, device):
    lib, p, ctx = fake
    for h, out, keys in [(None, p, p), (ctx, None, p), (ctx, p, None)]:
        # a bad kind, components == 0 and count == 0 do not come first
        for count, kind, param, components in [(1, 0, 0, 1), (0, 0, 0, 1), (1, 7, 0, 1), (1, 0, 0, 0), (0, -1, 5, 0)]:
            assert _sample(lib, device, h, out, count, kind, param, keys, components) == -1
            msg = pkg._abi.last_error()
            assert "NULL" in msg and msg.startswith(_name(device) + ":"), msg


@pytest.mark.parametrize("device", [False, True])
def test_kind_then_components_come_before_anything_that_reads_the_context(pkg, fake, device):
    """The context is fake: reading q or n from it would give nonsense, not these messages.  Also for count == 0, which is looked at
    later, and with a param no kind takes."""
    lib, p, ctx = fake
    for kind in (3, -1, 64, 2**31 - 1):
        for count, param, components in [(1, 0, 1), (0, 0, 1), (1, 2**64 - 1, 0), (0, 1, 0)]:
            assert _sample(lib, device, ctx, p, count, kind, param, p, components) == -1
            msg = pkg._abi.last_error()
            assert "kind" in msg and msg.startswith(_name(device) + ":"), msg
    for kind in (model.UNIFORM, model.BOUNDED, model.BALL):
        for count, param in [(1, 0), (0, 0), (1, 2**64 - 1), (0, 1)]:
            assert _sample(lib, device, ctx, p, count, kind, param, p, 0) == -1
            msg = pkg._abi.last_error()
            assert "components" in msg and "kind" not in msg and msg.startswith(_name(device) + ":"), msg


def test_seeded_matrix_refusals_that_read_no_context(pkg, fake):
    """lsr_ntt_ring_matrix_create's order with the key in the place of m: NULL, rows == 0, cols == 0, rows over its cap, cols over its
    cap, rows * cols over the byte cap at any n."""
    lib, p, ctx = fake
    create = lib.lsr_ntt_ring_matrix_create_seeded
    for h, key in [(None, p), (ctx, None)]:
        for rows, cols in [(1, 1), (0, 3)]:
            assert not create(h, key, 16, 0, rows, cols)
            msg = pkg._abi.last_error()
            assert "NULL" in msg and msg.startswith("lsr_ntt_ring_matrix_create_seeded:"), msg
    big_rows, big_cols = pkg.RING_MATVEC_MAX_ROWS + 1, pkg.RING_DOT_MAX_TERMS + 1
    for rows, cols, named in [(0, 3, "rows"), (3, 0, "cols"), (0, 0, "rows"), (big_rows, 1, "rows"), (1, big_cols, "cols"), (0, big_cols, "rows"),
                              (big_rows, 0, "cols")]:
        for index_base in (0, 2**64 - 1):                       # the index overflow is looked at later
            assert not create(ctx, p, 16, index_base, rows, cols), (rows, cols)
            msg = pkg._abi.last_error()
            other = "cols" if named == "rows" else "rows"
            assert named in msg and other not in msg and msg.startswith("lsr_ntt_ring_matrix_create_seeded:"), (rows, cols, msg)
    rows, cols = pkg.RING_MATVEC_MAX_ROWS, pkg.RING_MATVEC_MAX_MATRIX_BYTES // 16 // pkg.RING_MATVEC_MAX_ROWS + 1
    assert not create(ctx, p, 16, 0, rows, cols) and "LSR_RING_MATVEC_MAX_MATRIX_BYTES" in pkg._abi.last_error()


def test_python_wrapper_checks_the_key_count_before_the_library_reads_it(pkg):
    """ring_sample must not hand the library fewer keys than ceil(count / components): it would read past the array."""
    class Ctx(pkg._RingSample):
        n, _h, _lib = 16, None, None
    with pytest.raises(ValueError, match="ceil"):
        Ctx().ring_sample(5, pkg.RING_SAMPLE_UNIFORM, 0, np.zeros((2, 4), dtype=np.uint64), components=2)
    with pytest.raises(ValueError, match="32 bytes"):
        Ctx().ring_sample(1, pkg.RING_SAMPLE_UNIFORM, 0, b"short")
    with pytest.raises(ValueError, match="four"):
        Ctx().ring_sample(1, pkg.RING_SAMPLE_UNIFORM, 0, np.zeros(3, dtype=np.uint64))
