"""CPU suite: the bounded resident-matrix product under an arbitrary modulus (lsr_ring_mod_matvec_bounded_batch, batch.h "resident
matrices under any modulus") is declared with its contract, exported and mirrored in ctypes and in RingModMatrix; the
refusals that need no device come in batch.h's order; and the grouping rule, which is host arithmetic, gives the group counts the
model predicts.

The matrix handles of the refusal tests are fake and never used as handles: those refusals read only the leading fields the
structure documents (q, rows, cols, n), and every call made here is refused before any device work — also on a machine with a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import ring_mod_matvec_bounded_model as model
import ring_mod_matvec_model as matvec_model
from ring_mod_matvec_bounded_model import (test_model_groups,  # noqa: F401  (collected here: the model's own tests)
                                           test_model_matvec_bounded_gates_whole_vectors)  # noqa: F401
from test_ring_mod_matvec_abi import Fake

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_H = os.path.join(ROOT, "include", "lambda_snark", "batch.h")
ARGUMENTS = {
    "lsr_ring_mod_matvec_bounded_batch": ["mat", "y", "status", "x", "batch", "bound_x"],
    "lsr_ring_mod_matvec_bounded_batch_device": ["mat", "d_y", "d_status", "d_x", "batch", "bound_x", "stream"],
}
Q40 = model.Q40


def test_batch_h_declares_the_functions_in_their_section_with_the_contract():
    raw = open(BATCH_H).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, want in ARGUMENTS.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*LSR_NOEXCEPT", text)
        assert m, name
        assert [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")] == want, name
    # in the section of the resident matrices, behind the products it extends
    assert text.index("lsr_ring_mod_matvec_gadget_batch_device") < text.index("lsr_ring_mod_matvec_bounded_batch") \
        < text.index("lsr_ring_mod_matvec_bounded_batch_device") < text.index("lsr_ring_mod_capacity_product")
    section = raw[raw.index("resident matrices under any modulus"):raw.index("Gram matrices under any modulus")]
    for word in ("The bounded product", "status [batch] (int32), never NULL", "0 states none, which is floor(q/2)", "(-1 wins over 0)",
                 "EVERY word of y[j] is 0", "lsr_ring_mod_capacity_bounded(q, n, bound_x)", "verified, not promised",
                 "A violation found in a later group still leaves y[j] all zero", "bound_x above floor(q/2)", "status overlapping",
                 "from the first call", "capped at 4096 vectors", "lsr_ring_mod_fold_batch at width = 1, term_stride = terms"):
        assert word in section, word                            # the definition is the contract and lives in the header


def test_library_exports_signatures_and_members(pkg):
    lib = pkg._abi.load_library()
    u64, vp, size = ctypes.c_uint64, ctypes.c_void_p, ctypes.c_size_t
    want = {"lsr_ring_mod_matvec_bounded_batch": [vp, vp, vp, vp, size, u64],
            "lsr_ring_mod_matvec_bounded_batch_device": [vp, vp, vp, vp, size, u64, vp]}
    for name, args in want.items():
        assert hasattr(lib, name), name
        assert pkg._abi.SIGNATURES[name][0] is ctypes.c_int
        assert list(pkg._abi.SIGNATURES[name][1]) == args, name
        assert len(args) == len(ARGUMENTS[name])
    for member in ("matvec_bounded", "matvec_bounded_device"):
        assert hasattr(pkg.RingModMatrix, member), member


@pytest.fixture()
def fake(pkg):
    return Fake(pkg)


@pytest.mark.parametrize("name,device", [("lsr_ring_mod_matvec_bounded_batch", False), ("lsr_ring_mod_matvec_bounded_batch_device", True)])
def test_refusals_in_the_documented_order(fake, name, device):
    f = fake
    status_buf = (ctypes.c_int32 * 16)()
    st = ctypes.addressof(status_buf)

    def call(mat, y, status, x, batch=1, bound=0):
        return getattr(f.lib, name)(*([mat, y, status, x, batch, bound] + ([None] if device else [])))

    def refused(word, *args, **kw):
        assert call(*args, **kw) == -1
        msg = f.message(name)
        assert word in msg, msg
        return msg

    q, n = 3329, 4
    f.matrix(q, 2, 3, n)                                       # y [1][2][4], x [1][3][4]
    # (1) NULL, before the bound and before the empty call
    for mat, y, status, x in [(None, f.c, st, f.a), (f.mat, None, st, f.a), (f.mat, f.c, None, f.a), (f.mat, f.c, st, None)]:
        for kw in [{}, dict(batch=0), dict(bound=q // 2 + 1), dict(bound=2**64 - 1, batch=0)]:
            refused("NULL", mat, y, status, x, **kw)
    # (2) bound_x above floor(q/2), before the empty call and before the overlaps
    for kw in [dict(bound=q // 2 + 1), dict(bound=q // 2 + 1, batch=0), dict(bound=2**64 - 1)]:
        msg = refused("above floor(q / 2) = 1664", f.mat, f.a, f.a, f.a, **kw)
        assert "bound_x = %d" % kw["bound"] in msg
    # (3) the empty call is a no-op, whatever overlaps — also at the largest bound
    assert call(f.mat, f.a, f.a, f.a, batch=0) == 0
    assert call(f.mat, f.a, f.a, f.a, batch=0, bound=q // 2) == 0
    # (4) y overlapping x, also in part, before (5)
    for y in (f.a, f.a + 8, f.a + 8 * (3 * n - 1)):
        refused("y overlaps x", f.mat, y, f.a, f.a)            # (status overlaps x as well: y comes first)
    refused("y overlaps x", f.mat, f.a, st, f.a + 8 * (2 * n - 1), bound=q // 2)
    # (5) status overlapping x, then y: one int32 per vector
    refused("status overlaps x", f.mat, f.c, f.a, f.a)
    refused("status overlaps x", f.mat, f.c, f.a + 8 * 3 * n - 4, f.a)
    refused("status overlaps y", f.mat, f.c, f.c, f.a)
    refused("status overlaps y", f.mat, f.c, f.c + 8 * 2 * n - 4, f.a)
    # (6) every refusal above needed no device; a call that passes them is refused on a machine without one
    if f.lib.lsr_device_count() <= 0:
        refused("no HIP device visible", f.mat, f.c, st, f.a)


def test_python_wrappers_check_the_shapes(pkg):
    class Lib:                                                 # rows and cols without a handle
        @staticmethod
        def lsr_ring_mod_matrix_rows(_):
            return 2

        @staticmethod
        def lsr_ring_mod_matrix_cols(_):
            return 3

    mat = pkg.RingModMatrix.__new__(pkg.RingModMatrix)
    mat._lib, mat._h, mat.n = Lib, None, 16
    for bad in (np.zeros(16, dtype=np.uint64), np.zeros((2, 16), dtype=np.uint64), np.zeros((1, 3, 8), dtype=np.uint64),
                np.zeros((1, 1, 3, 16), dtype=np.uint64)):
        with pytest.raises(ValueError, match=r"\[cols, n\] or \[batch, cols, n\]"):
            mat.matvec_bounded(bad)
    for bound in (-1, 2**64):
        with pytest.raises(ValueError, match="bound_x"):
            mat.matvec_bounded(np.zeros((3, 16), dtype=np.uint64), bound)


def test_grouping_rule_on_the_host(pkg):
    """q = 2^40 + 15, n = 64, 50 columns: 8 groups unbounded, 3 at floor(floor(q/2) / 3) (capacity 23), 1 at 128 — the library's
    capacity, which sizes the groups, is the model's"""
    q, n, h = Q40, 64, Q40 // 2
    assert len(model.groups(q, n, 50)) == 8
    assert matvec_model.capacity_bounded(q, n, h // 3) == 23 and model.groups(q, n, 50, h // 3) == [23, 23, 4]
    assert len(model.groups(q, n, 50, 128)) == 1
    for bound in (h, h // 3, 128):
        assert pkg.ring_mod_capacity_bounded(q, n, bound) == matvec_model.capacity_bounded(q, n, bound)
    assert pkg.ring_mod_capacity_bounded(q, n, h) == pkg.ring_mod_capacity(q, n) == 7      # bound_x = 0 reads as h: max_terms
    assert len(model.groups(q, n, 258)) == 37 and model.groups(q, n, 258, 128) == [258]
