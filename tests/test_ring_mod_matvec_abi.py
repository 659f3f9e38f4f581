"""CPU suite: the resident matrices under an arbitrary modulus (lsr_ring_mod_matrix_* / lsr_ring_mod_matvec_*, batch.h "resident
matrices under any modulus") are declared, exported and mirrored in ctypes and in RingMod / RingModMatrix; the
host-only capacity with a short operand agrees with the Python-integer model (tests/ring_mod_matvec_model.py); and the refusals that
need no device come in batch.h's order, so they answer NULL or -1 with a message on a machine without a GPU.

The handles of the refusal tests are fake and never used as handles: those refusals read only the leading fields the structures
document (LsrRingMod: q, n; LsrRingModMatrix: q, rows, cols, n), and every call made here is refused before any device work — also
on a machine that has a GPU."""
import ctypes
import os
import re

import pytest

import ring_gadget_model as gadget
import ring_mod_matvec_model as model
import ring_mod_model as mod
from ring_mod_matvec_model import (test_model_capacity_bounded,  # noqa: F401  (collected here: the model's own tests)
                                   test_model_matvec_is_the_schoolbook_and_the_gadget_recomposes)  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_H = os.path.join(ROOT, "include", "lambda_snark", "batch.h")
ARGUMENTS = {
    "lsr_ring_mod_capacity_bounded": ["q", "n", "bound"],
    "lsr_ring_mod_matrix_create": ["h", "m", "rows", "cols"],
    "lsr_ring_mod_matrix_create_device": ["h", "d_m", "rows", "cols", "stream"],
    "lsr_ring_mod_matrix_create_seeded": ["h", "key[4]", "domain", "index_base", "rows", "cols"],
    "lsr_ring_mod_matrix_free": ["mat"],
    "lsr_ring_mod_matrix_rows": ["mat"],
    "lsr_ring_mod_matrix_cols": ["mat"],
    "lsr_ring_mod_matrix_row_block": ["mat"],
    "lsr_ring_mod_matvec_batch": ["mat", "y", "x", "batch"],
    "lsr_ring_mod_matvec_batch_device": ["mat", "d_y", "d_x", "batch", "stream"],
    "lsr_ring_mod_matvec_gadget_batch": ["mat", "y", "x", "batch", "base_log2", "digits"],
    "lsr_ring_mod_matvec_gadget_batch_device": ["mat", "d_y", "d_x", "batch", "base_log2", "digits", "stream"],
}
MATRIX_MEMBERS = ("rows", "cols", "row_block", "matvec", "matvec_device", "matvec_gadget", "matvec_gadget_device", "close", "__enter__", "__exit__")
MAX_ROWS, MAX_COLS, MAX_BYTES = 32768, 65536, 1 << 30
Q40 = (1 << 40) + 15


def test_batch_h_declares_the_functions_in_their_section_with_the_contract():
    raw = open(BATCH_H).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, want in ARGUMENTS.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*LSR_NOEXCEPT", text)
        assert m, name
        assert [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")] == want, name
    assert "typedef struct LsrRingModMatrix LsrRingModMatrix;" in text
    # after the fused products of the handle, before the Gaussian sampler
    assert text.index("lsr_ring_mod_dot_batch_device") < text.index("typedef struct LsrRingModMatrix") \
        < text.index("lsr_ring_mod_matvec_gadget_batch_device") < text.index("lsr_sample_gaussian_seeded")
    for word in ("floor(((P - 1)/2) / (n floor(q/2) bound))", "lsr_ring_mod_capacity_bounded(q, n, B/2)", "at most max_terms", "taken against q",
                 "lsr_ring_gadget_min_digits(q, b)", "index_base + r cols + c", "rows cols 16 above the byte cap", "cols % digits != 0",
                 "from the first call", "must outlive"):
        assert word in raw, word                               # the definition is the contract and lives in the header


def test_library_exports_signatures_and_members(pkg):
    lib = pkg._abi.load_library()
    for name, want in ARGUMENTS.items():
        assert hasattr(lib, name), name
        assert len(pkg._abi.SIGNATURES[name][1]) == len(want), name
    for name in ("lsr_ring_mod_matrix_create", "lsr_ring_mod_matrix_create_device", "lsr_ring_mod_matrix_create_seeded"):
        assert pkg._abi.SIGNATURES[name][0] is ctypes.c_void_p
    for name in ("lsr_ring_mod_capacity_bounded", "lsr_ring_mod_matrix_rows", "lsr_ring_mod_matrix_cols", "lsr_ring_mod_matrix_row_block"):
        assert pkg._abi.SIGNATURES[name][0] is ctypes.c_size_t
    assert pkg._abi.SIGNATURES["lsr_ring_mod_matrix_free"][0] is None
    for member in ("matrix", "matrix_device", "matrix_seeded"):
        assert hasattr(pkg.RingMod, member), member
    for member in MATRIX_MEMBERS:
        assert hasattr(pkg.RingModMatrix, member), member
    for name in ("RingModMatrix", "ring_mod_capacity_bounded"):
        assert name in pkg.__all__


def _moduli():
    p5 = mod.prime_5_mod_8_below(1 << 32)
    top = mod.largest_admissible(64)
    return [2, 3, 3329, 1 << 23, p5, 1 << 32, (1 << 40) - 87, Q40, top, top + 1]


def test_capacity_bounded_is_the_models(pkg):
    for q in _moduli():
        for n in (2, 64, 256, 4096):
            for bound in (0, 1, 8, 1 << 31, q // 2, q // 2 + 1):
                assert pkg.ring_mod_capacity_bounded(q, n, bound) == model.capacity_bounded(q, n, bound), (q, n, bound)


def test_capacity_bounded_identity_saturation_and_zeros(pkg):
    for q in _moduli() + [0, 1, 4, 5, (1 << 44) + 1, 2**64 - 1]:
        for n in (2, 64, 256, 4096, 65536, 131072, 0, 3):
            assert pkg.ring_mod_capacity_bounded(q, n, q // 2) == pkg.ring_mod_capacity(q, n), (q, n)
            if pkg.ring_mod_capacity(q, n) == 0:
                assert pkg.ring_mod_capacity_bounded(q, n, 1) == 0, (q, n)
    assert pkg.ring_mod_capacity_bounded(2, 64, 1) == 2**64 - 1 == pkg.ring_mod_capacity_bounded(3, 64, 1)          # saturated
    assert pkg.ring_mod_capacity_bounded(2, 64, 2) == 0 and pkg.ring_mod_capacity_bounded(2, 64, 2**64 - 1) == 0
    assert pkg.ring_mod_capacity_bounded(Q40, 64, 1 << 31) == 2047 and pkg.ring_mod_capacity(Q40, 64) == 7
    assert pkg.ring_mod_capacity_bounded(Q40, 64, 128) == model.capacity_bounded(Q40, 64, 128) == 34359705185
    assert pkg.ring_mod_capacity_bounded(2**64, 64, 1) == 0 and pkg.ring_mod_capacity_bounded(3329, 64, -1) == 0     # the wrapper's range check


class Fake:
    """The library, buffers apart from each other, a ring handle and a matrix handle of zeros with their leading fields settable."""

    def __init__(self, pkg):
        self.pkg, self.lib = pkg, pkg._abi.load_library()
        self.bufs = [(ctypes.c_uint64 * 64)() for _ in range(3)]
        self.h_buf = (ctypes.c_uint64 * 256)()
        self.m_buf = (ctypes.c_uint64 * 64)()
        self.a, self.b, self.c = (ctypes.addressof(b) for b in self.bufs)
        self.h, self.mat = ctypes.addressof(self.h_buf), ctypes.addressof(self.m_buf)

    def ring(self, q, n):
        self.h_buf[0], self.h_buf[1] = q, n                    # uint64 q; uint32 n (little-endian: the low half of word 1)

    def matrix(self, q, rows, cols, n):
        self.m_buf[0], self.m_buf[1], self.m_buf[2], self.m_buf[3] = q, rows, cols, n

    def message(self, name):
        msg = self.pkg._abi.last_error()
        assert msg.startswith(name + ":"), msg
        return msg


@pytest.fixture()
def fake(pkg):
    return Fake(pkg)


@pytest.mark.parametrize("name", ["lsr_ring_mod_matrix_create", "lsr_ring_mod_matrix_create_device", "lsr_ring_mod_matrix_create_seeded"])
def test_create_refusals_in_the_documented_order(fake, name):
    f = fake
    seeded, device = name.endswith("seeded"), name.endswith("device")

    def call(h, m, rows, cols, index_base=0):
        if seeded:
            return f.lib.lsr_ring_mod_matrix_create_seeded(h, m, 16, index_base, rows, cols)
        return getattr(f.lib, name)(*([h, m, rows, cols] + ([None] if device else [])))

    def refused(word, *args, **kw):
        assert not call(*args, **kw)
        msg = f.message(name)
        assert word in msg, msg
        return msg

    f.ring(3329, 8192)                                        # every later step would refuse too
    # (1) NULL
    for h, m in [(None, f.a), (f.h, None)]:
        for rows, cols in [(1, 1), (0, 0), (MAX_ROWS + 1, MAX_COLS + 1)]:
            refused("NULL", h, m, rows, cols)
    # (2) rows == 0 before (3) cols == 0 before the caps
    refused("rows must be at least 1", f.h, f.a, 0, 0)
    refused("rows must be at least 1", f.h, f.a, 0, MAX_COLS + 1)
    refused("cols must be at least 1", f.h, f.a, MAX_ROWS + 1, 0)
    # (4) rows above its cap before (5) cols above its cap
    refused("LSR_RING_MATVEC_MAX_ROWS", f.h, f.a, MAX_ROWS + 1, MAX_COLS + 1)
    refused("LSR_RING_DOT_MAX_TERMS", f.h, f.a, MAX_ROWS, MAX_COLS + 1)
    # (6) rows cols 16 above the byte cap: over it at any n
    msg = refused("at any n", f.h, f.a, MAX_ROWS, MAX_COLS)
    assert "4096" not in msg
    assert MAX_ROWS * 2049 * 16 > MAX_BYTES
    refused("at any n", f.h, f.a, MAX_ROWS, 2049)
    # (7) n above 4096, with the composed route, before (8)
    for rows, cols in [(1, 1), (MAX_ROWS, 2048)]:
        msg = refused("above 4096", f.h, f.a, rows, cols)
        for word in ("lsr_ring_mod_lift_batch_device", "lsr_ntt_ring_matrix_create_device", "lsr_ring_mod_prime_context", "lsr_ntt_ring_matvec_batch_device",
                     "lsr_ring_mod_reduce_batch_device", "lsr_ring_mod_max_terms"):
            assert word in msg, msg
    # (8) rows cols n 8 above the byte cap, before (9)
    f.ring(3329, 4096)
    assert 64 * 513 * 4096 * 8 > MAX_BYTES >= 64 * 512 * 4096 * 8
    msg = refused("LSR_RING_MATVEC_MAX_MATRIX_BYTES", f.h, f.a, 64, 513, index_base=2**64 - 1)
    assert "rows * cols * n * 8" in msg
    # (9) seeded: the stream indices must not wrap
    if seeded:
        f.ring(3329, 64)
        refused("overflows 64 bits", f.h, f.a, 3, 5, index_base=2**64 - 15)
        refused("overflows 64 bits", f.h, f.a, 1, 1, index_base=2**64 - 1)


def test_free_and_accessors_are_null_safe(pkg, fake):
    lib = fake.lib
    lib.lsr_ring_mod_matrix_free(None)
    assert lib.lsr_ring_mod_matrix_rows(None) == 0 and lib.lsr_ring_mod_matrix_cols(None) == 0 and lib.lsr_ring_mod_matrix_row_block(None) == 0
    fake.matrix(3329, 5, 7, 64)
    assert lib.lsr_ring_mod_matrix_rows(fake.mat) == 5 and lib.lsr_ring_mod_matrix_cols(fake.mat) == 7


@pytest.mark.parametrize("name,device,is_gadget", [("lsr_ring_mod_matvec_batch", False, False), ("lsr_ring_mod_matvec_batch_device", True, False),
                                                   ("lsr_ring_mod_matvec_gadget_batch", False, True),
                                                   ("lsr_ring_mod_matvec_gadget_batch_device", True, True)])
def test_product_refusals_in_the_documented_order(fake, name, device, is_gadget):
    f = fake

    def call(mat, y, x, batch=1, b=4, digits=3):
        args = [mat, y, x, batch] + ([b, digits] if is_gadget else []) + ([None] if device else [])
        return getattr(f.lib, name)(*args)

    def refused(word, *args, **kw):
        assert call(*args, **kw) == -1
        msg = f.message(name)
        assert word in msg, msg
        return msg

    q, n = 3329, 4
    assert gadget.min_digits(q, 4) == 3 and not gadget.admissible(q, 4, 2) and gadget.min_digits(q, 12) == 0
    f.matrix(q, 2, 7, n)                                       # cols 7: no multiple of 3 digits
    # (1) NULL, before everything that follows and before the empty call
    for mat, y, x in [(None, f.c, f.a), (f.mat, None, f.a), (f.mat, f.c, None)]:
        for kw in [{}, dict(batch=0), dict(b=1), dict(digits=0), dict(b=4, digits=2)]:
            refused("NULL", mat, y, x, **kw)
    if is_gadget:
        # (2) the shape of (b, D), before admissibility, the divisibility and the empty call
        for kw, word in [(dict(b=1), "outside [2, 32]"), (dict(b=33, batch=0), "outside [2, 32]"), (dict(digits=0), "digits must be at least 1"),
                         (dict(b=4, digits=17, batch=0), "above 64"), (dict(b=32, digits=3), "above 64")]:
            refused(word, f.mat, f.c, f.a, **kw)
        # (3) admissibility for the matrix's q, before the divisibility and the empty call
        for kw in [dict(b=4, digits=2), dict(b=4, digits=2, batch=0), dict(b=12, digits=1), dict(b=12, digits=5)]:
            msg = refused("not admissible for q = 3329", f.mat, f.c, f.a, **kw)
            assert "lsr_ring_gadget_min_digits gives " + str(gadget.min_digits(q, kw["b"])) in msg, msg
        # (4) cols % digits, before the empty call
        refused("not a multiple of digits", f.mat, f.c, f.a, b=4, digits=3)
        refused("not a multiple of digits", f.mat, f.c, f.a, b=4, digits=3, batch=0)
        f.matrix(q, 2, 6, n)
    # (5) the empty call is a no-op, whatever overlaps
    assert call(f.mat, f.a, f.a, batch=0) == 0
    # (6) y overlapping x in address range: y [1][2][4] against x [1][cols or xcols][4], also in part
    for y in (f.a, f.a + 8, f.a + 8 * (2 * n - 1)):
        refused("y overlaps x", f.mat, y, f.a + 8 * (2 * n - 1) if y == f.a else f.a)


def test_python_wrappers_check_the_shapes(pkg):
    import numpy as np
    ring = pkg.RingMod.__new__(pkg.RingMod)
    ring.n, ring._h, ring._lib = 16, None, None
    with pytest.raises(ValueError, match="rows, cols, n"):
        ring.matrix(np.zeros((3, 16), dtype=np.uint64))
    with pytest.raises(ValueError, match="256-bit"):
        ring.matrix_seeded(np.zeros(8, dtype=np.uint64), 16, 0, 1, 1)


class _RecordingLib:
    """stands in for the library: records which handle each free receives, in order"""

    def __init__(self):
        self.calls = []

    def lsr_ring_mod_matrix_free(self, handle):
        self.calls.append(("matrix", handle))

    def lsr_ring_mod_free(self, handle):
        self.calls.append(("ring", handle))


def _recorded_ring(pkg):
    import weakref
    lib = _RecordingLib()
    ring = pkg.RingMod.__new__(pkg.RingMod)
    ring.n, ring._h, ring._lib = 16, 1000, lib
    ring._contexts, ring._matrices, ring._matrix_handles = [None, None, None], weakref.WeakSet(), set()
    return lib, ring


def test_every_matrix_is_freed_once_and_before_its_ring_in_either_close_order(pkg):
    """lsr_ring_mod_matrix_free reads the ring's handle, so no matrix may be freed after lsr_ring_mod_free.  The ring finds live matrices
    through a WeakSet; when ring and matrices are collected as cyclic garbage (a failed test's traceback holds both) the weak references
    are cleared before any finalizer runs and the ring's may run first: cleared here by hand, as the collector does."""
    lib, ring = _recorded_ring(pkg)                      # the usual order: matrix, then ring
    a, b = pkg.RingModMatrix(ring, 1), pkg.RingModMatrix(ring, 2)
    a.close()
    a.close()
    ring.close()
    b.close()
    assert lib.calls == [("matrix", 1), ("matrix", 2), ("ring", 1000)] and a.handle is None and b.handle is None

    lib, ring = _recorded_ring(pkg)                      # the collector's order: weak references gone, the ring's finalizer first
    a, b = pkg.RingModMatrix(ring, 1), pkg.RingModMatrix(ring, 2)
    ring._matrices.clear()
    ring.close()
    assert sorted(lib.calls[:2]) == [("matrix", 1), ("matrix", 2)] and lib.calls[2:] == [("ring", 1000)]
    a.close()
    del b                                                # RingModMatrix.__del__
    assert len(lib.calls) == 3 and a.handle is None
    ring.close()
    assert len(lib.calls) == 3
