"""CPU suite: the ring quadratic forms under an arbitrary modulus (lsr_ring_mod_quadform_*, batch.h "quadratic forms under any
modulus") are declared, exported and mirrored in ctypes and in RingMod; the host-only capacity of a cubic sum agrees
with the Python-integer model (tests/ring_mod_quadform_model.py) and with the pinned table; and the refusals that need no device come
in batch.h's order, so they answer -1 with a message on a machine without a GPU.

The handle of the refusal tests is fake and never used as a handle: those refusals read only the leading fields LsrRingMod documents
(q, n; logn is the third), and every call made here is refused before any device work — also on a machine that has a GPU."""
import ctypes
import os
import re

import pytest

import ring_mod_model as mod
import ring_mod_quadform_model as model
from ring_mod_quadform_model import (test_model_capacity_quadform_table_zeros_and_the_group_rule,  # noqa: F401  (collected here: the model's own tests)
                                     test_model_quadform_is_the_schoolbook_pair_by_pair_and_the_status_gates)  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_H = os.path.join(ROOT, "include", "lambda_snark", "batch.h")
ARGUMENTS = {
    "lsr_ring_mod_capacity_quadform": ["q", "n", "bound_g", "bound_c"],
    "lsr_ring_mod_quadform_batch": ["h", "out", "status", "g", "c", "batch", "r", "c_rows", "offdiag", "bound_g", "bound_c"],
    "lsr_ring_mod_quadform_batch_device": ["h", "d_out", "d_status", "d_g", "d_c", "batch", "r", "c_rows", "offdiag", "bound_g", "bound_c", "stream"],
}
MAX_VECTORS = 64
Q40 = (1 << 40) + 15
P5 = 4294967197
CALLS = ["lsr_ring_mod_quadform_batch", "lsr_ring_mod_quadform_batch_device"]


def test_batch_h_declares_the_functions_in_their_section_with_the_contract():
    raw = open(BATCH_H).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, want in ARGUMENTS.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*LSR_NOEXCEPT", text)
        assert m, name
        assert [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")] == want, name
    # after the fold of the handle, before the Gaussian sampler
    assert text.index("lsr_ring_mod_fold_batch_device") < text.index("lsr_ring_mod_capacity_quadform") \
        < text.index("lsr_ring_mod_quadform_batch_device") < text.index("lsr_sample_gaussian_seeded")
    for word in ("floor(((P - 1)/2) / (n^2 bound_g bound_c^2))", "-1 wins over 0", "EVERY word of out[j] is 0", "A bound of 0 states none", "CUBIC",
                 "W = max(1, |w|)", "gates every\n * family", "gates family j alone", "names bound_c", "lsr_ring_mod_mul_batch per pair",
                 "lsr_ring_mod_gram_prepare(h)", "r + 3 polynomials", "g and c are never written", "refused on the handle's coefficient context"):
        assert word in raw, word                               # the definition is the contract and lives in the header


def test_library_exports_signatures_and_members(pkg):
    lib = pkg._abi.load_library()
    for name, want in ARGUMENTS.items():
        assert hasattr(lib, name), name
        assert len(pkg._abi.SIGNATURES[name][1]) == len(want), name
    assert pkg._abi.SIGNATURES["lsr_ring_mod_capacity_quadform"][0] is ctypes.c_size_t
    for name in CALLS:
        assert pkg._abi.SIGNATURES[name][0] is ctypes.c_int
    for member in ("quadform", "quadform_device", "gram_prepare"):
        assert hasattr(pkg.RingMod, member), member
    assert "ring_mod_capacity_quadform" in pkg.__all__


def test_capacity_quadform_table(pkg):
    for q, n, bound_g, bound_c, want in model.CAPACITY_TABLE:
        assert pkg.ring_mod_capacity_quadform(q, n, bound_g, bound_c) == want, (q, n, bound_g, bound_c)
    assert model.SIZE_MAX == 2**64 - 1 == pkg.ring_mod_capacity_quadform(Q40, 64, 128, 2)


def _moduli():
    top = mod.largest_admissible(64)
    return [2, 3, 3329, 1 << 23, P5, 1 << 32, (1 << 40) - 87, Q40, 8246337208321, top, top + 1]


def test_capacity_quadform_is_the_models_on_a_grid(pkg):
    """the grid holds the bounds 0, 1, h and h + 1 and (q, n) of capacity 0 (top + 1 at n = 64, most moduli at n = 4096, n = 3)"""
    zero = nonzero = 0
    for q in _moduli():
        h = q // 2
        for n in (2, 8, 64, 256, 4096, 65536, 3):
            zero += mod.capacity(q, n) == 0
            bounds = sorted({0, 1, 2, 128, min(1 << 20, h), h, h + 1})
            for bg in bounds:
                for bc in bounds:
                    want = model.capacity_quadform(q, n, bg, bc)
                    assert pkg.ring_mod_capacity_quadform(q, n, bg, bc) == want, (q, n, bg, bc)
                    nonzero += want != 0
    assert zero >= 3 and nonzero >= 100
    for q, n in [(0, 64), (1, 64), (3329, 0), (3329, 3), (3329, 1 << 18)]:
        assert pkg.ring_mod_capacity_quadform(q, n, 1, 1) == 0, (q, n)
    assert pkg.ring_mod_capacity_quadform(2**64, 64, 1, 1) == 0 and pkg.ring_mod_capacity_quadform(3329, 64, -1, 1) == 0     # the wrapper's range check


class Fake:
    """The library, buffers apart from each other and a ring handle of zeros with its leading fields settable."""

    def __init__(self, pkg):
        self.pkg, self.lib = pkg, pkg._abi.load_library()
        self.bufs = [(ctypes.c_uint64 * 1024)() for _ in range(4)]
        self.h_buf = (ctypes.c_uint64 * 512)()
        self.out, self.g, self.c, self.status = (ctypes.addressof(b) for b in self.bufs)
        self.h = ctypes.addressof(self.h_buf)

    def ring(self, q, n):
        self.h_buf[0] = q
        self.h_buf[1] = n | (n.bit_length() - 1) << 32         # uint32 n, int logn (little-endian: the two halves of word 1)

    def message(self, name):
        msg = self.pkg._abi.last_error()
        assert msg.startswith(name + ":"), msg
        return msg


@pytest.fixture()
def fake(pkg):
    return Fake(pkg)


@pytest.mark.parametrize("name", CALLS)
def test_refusals_without_a_device_in_the_documented_order(fake, name):
    f = fake
    device = name.endswith("device")

    def call(h, out, status, g, c, batch=1, r=2, c_rows=None, offdiag=2, bound_g=0, bound_c=2):
        args = [h, out, status, g, c, batch, r, batch if c_rows is None else c_rows, offdiag, bound_g, bound_c] + ([None] if device else [])
        return getattr(f.lib, name)(*args)

    def refused(word, *args, **kw):
        assert call(*args, **kw) == -1
        msg = f.message(name)
        assert word in msg, msg
        return msg

    q = 3329
    f.ring(q, 4)
    h = q // 2
    ok = (f.h, f.out, f.status, f.g, f.c)
    # (1) NULL h, out, status, g or c, whatever the shape
    for k in range(5):
        args = ok[:k] + (None,) + ok[k + 1:]
        refused("NULL", *args)
        refused("NULL", *args, r=0, c_rows=3, offdiag=q, bound_g=h + 1)
    # (2) r == 0 before (3) c_rows, (3) before (4) the cap, (4) before (5) the sizes, (5) before (6) offdiag, (6) before (7) the bounds
    refused("at least 1", *ok, r=0, c_rows=3, offdiag=q)
    msg = refused("c_rows must be 1", *ok, batch=4, r=MAX_VECTORS + 1, c_rows=3)
    assert "c_rows = 3" in msg and "batch = 4" in msg
    refused("LSR_RING_GRAM_MAX_VECTORS", *ok, batch=2**60, r=MAX_VECTORS + 1, offdiag=q)
    refused("overflow", *ok, batch=2**60, offdiag=q, bound_c=h + 1)
    msg = refused("offdiag", *ok, offdiag=q, bound_c=h + 1)
    assert "canonical" in msg and str(q) in msg
    refused("offdiag", *ok, batch=0, c_rows=1, offdiag=2**64 - 1)
    # (7) a bound above floor(q / 2), before the empty call and before the overlap
    for kw in ({"bound_g": h + 1}, {"bound_c": h + 1}, {"bound_g": 2**64 - 1, "bound_c": 1}):
        msg = refused("above floor(q / 2)", *ok, batch=0, c_rows=1, **kw)
        assert str(h) in msg
    refused("above floor(q / 2)", f.h, f.g, f.status, f.g, f.c, bound_g=h + 1)
    # (8) the empty call is a no-op — with either c_rows, overlapping buffers and the largest admissible arguments
    assert call(f.h, f.g, f.status, f.g, f.c, batch=0, c_rows=1, offdiag=q - 1, bound_g=h, bound_c=h) == 0
    assert call(f.h, f.g, f.status, f.g, f.c, batch=0, c_rows=0) == 0
    # (9) family bytes before (10) the capacity
    f.ring(1 << 32, 131072)
    refused("LSR_RING_GRAM_MAX_FAMILY_BYTES", f.h, f.g, f.status, f.g, f.c, r=64, bound_c=0)
    # (10) the capacity: unbounded challenges at a 32-bit modulus, and an offdiag of (q + 1) / 2 at a large q — before (11) and (12)
    f.ring(P5, 64)
    msg = refused("bound_c", f.h, f.g, f.status, f.g, f.c, bound_c=0)
    assert "lsr_ring_mod_mul_batch" in msg and "lsr_ring_mod_dot_batch" in msg and "lsr_ring_mod_capacity_quadform" in msg
    f.ring(Q40, 64)
    msg = refused("bound_c", f.h, f.g, f.status, f.g, f.c, offdiag=(Q40 + 1) // 2)
    assert "lsr_ring_mod_mul_batch" in msg and str(Q40 // 2) in msg
    # (11) r + 3 polynomials per prime cannot be missed at the present limits, so no call reaches that refusal: a prime's half holds at
    # least 2^23 / 131072 = 64 polynomials, and a family of r >= 62 at that n is above LSR_RING_GRAM_MAX_FAMILY_BYTES, which (9) takes
    f.ring(1 << 23, 131072)
    refused("LSR_RING_GRAM_MAX_FAMILY_BYTES", f.h, f.g, f.status, f.g, f.c, r=62)
    assert 44 * 45 // 2 * 131072 * 8 <= 1 << 30 < 45 * 46 // 2 * 131072 * 8 and 44 + 3 <= 64
    # (12) overlaps: out and an operand, status and an operand, status and out — before the device
    f.ring(3329, 4)
    refused("out overlaps g", f.h, f.g, f.status, f.g, f.c)
    refused("out overlaps c", f.h, f.c + 8, f.status, f.g, f.c)
    refused("status overlaps g", f.h, f.out, f.g + 64, f.g, f.c)
    refused("status overlaps c", f.h, f.out, f.c, f.g, f.c)
    refused("status overlaps out", f.h, f.out, f.out + 16, f.g, f.c)
    # a shared c is one family's r polynomials: an out that starts in its last word overlaps it
    refused("out overlaps c", f.h, f.c + 2 * 4 * 8 - 8, f.status, f.g, f.c, batch=3, c_rows=1)
