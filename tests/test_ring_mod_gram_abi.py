"""CPU suite: the Gram matrices of bounded ring vectors under an arbitrary modulus (lsr_ring_mod_gram_*, batch.h "Gram matrices under
any modulus") are declared, exported and mirrored in ctypes and in RingMod; the host-only capacity with two short
operands agrees with the Python-integer model (tests/ring_mod_gram_model.py); and the refusals that need no device come in batch.h's
order, so they answer -1 with a message on a machine without a GPU.

The handle of the refusal tests is fake and never used as a handle: those refusals read only the leading fields LsrRingMod documents
(q, n; logn is the third), and every call made here is refused before any device work — also on a machine that has a GPU."""
import ctypes
import os
import re

import pytest

import ring_mod_gram_model as model
import ring_mod_model as mod
from ring_mod_gram_model import (test_model_capacity_product_table_and_identities,  # noqa: F401  (collected here: the model's own tests)
                                 test_model_gram_is_the_schoolbook_and_the_status_gates)  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_H = os.path.join(ROOT, "include", "lambda_snark", "batch.h")
ARGUMENTS = {
    "lsr_ring_mod_capacity_product": ["q", "n", "bound_a", "bound_b"],
    "lsr_ring_mod_gram_prepare": ["h"],
    "lsr_ring_mod_gram_batch": ["h", "g", "status", "a", "b", "batch", "ra", "rb", "width", "bound_a", "bound_b"],
    "lsr_ring_mod_gram_batch_device": ["h", "d_g", "d_status", "d_a", "d_b", "batch", "ra", "rb", "width", "bound_a", "bound_b", "stream"],
    "lsr_ring_mod_gram_sym2_batch": ["h", "out", "status", "a", "b", "batch", "r", "width", "bound_a", "bound_b"],
    "lsr_ring_mod_gram_sym2_batch_device": ["h", "d_out", "d_status", "d_a", "d_b", "batch", "r", "width", "bound_a", "bound_b", "stream"],
}
MAX_VECTORS, MAX_TERMS = 64, 65536
Q40 = model.Q40
CALLS = ["lsr_ring_mod_gram_batch", "lsr_ring_mod_gram_batch_device", "lsr_ring_mod_gram_sym2_batch", "lsr_ring_mod_gram_sym2_batch_device"]


def test_batch_h_declares_the_functions_in_their_section_with_the_contract():
    raw = open(BATCH_H).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, want in ARGUMENTS.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*LSR_NOEXCEPT", text)
        assert m, name
        assert [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")] == want, name
    # after the resident matrices of the handle, before the Gaussian sampler
    assert text.index("lsr_ring_mod_matvec_gadget_batch_device") < text.index("lsr_ring_mod_capacity_product") \
        < text.index("lsr_ring_mod_gram_sym2_batch_device") < text.index("lsr_sample_gaussian_seeded")
    for word in ("floor(((P - 1)/2) / (n bound_a bound_b))", "-1 wins over 0", "EVERY output word of that family is 0", "0 states", "does not read bound_b",
                 "held against both bounds", "names the cross form", "max(2^23,", "lsr_ring_mod_gram_prepare(h)", "never resized",
                 "Exactness never depends on the caller knowing a capacity"):
        assert word in raw, word                               # the definition is the contract and lives in the header


def test_library_exports_signatures_and_members(pkg):
    lib = pkg._abi.load_library()
    for name, want in ARGUMENTS.items():
        assert hasattr(lib, name), name
        assert len(pkg._abi.SIGNATURES[name][1]) == len(want), name
    assert pkg._abi.SIGNATURES["lsr_ring_mod_capacity_product"][0] is ctypes.c_size_t
    for name in CALLS + ["lsr_ring_mod_gram_prepare"]:
        assert pkg._abi.SIGNATURES[name][0] is ctypes.c_int
    for member in ("gram", "gram_device", "gram_sym2", "gram_sym2_device", "gram_prepare"):
        assert hasattr(pkg.RingMod, member), member
    assert "ring_mod_capacity_product" in pkg.__all__


def _moduli():
    p5 = mod.prime_5_mod_8_below(1 << 32)
    top = mod.largest_admissible(64)
    return [2, 3, 3329, 1 << 23, p5, 1 << 32, (1 << 40) - 87, Q40, 8246337208321, top, top + 1]


def test_capacity_product_is_the_models(pkg):
    """the grid holds the bounds 0, 1, h and h + 1 and (q, n) of capacity 0 (top + 1 at n = 64, most moduli at n = 4096, n = 3)"""
    zero = 0
    for q in _moduli():
        h = q // 2
        for n in (2, 8, 64, 256, 4096, 3):
            zero += mod.capacity(q, n) == 0
            bounds = sorted({0, 1, 2, 128, min(1 << 20, h), h, h + 1})
            for ba in bounds:
                for bb in bounds:
                    assert pkg.ring_mod_capacity_product(q, n, ba, bb) == model.capacity_product(q, n, ba, bb), (q, n, ba, bb)
    assert zero >= 3


def test_capacity_product_identities_saturation_and_zeros(pkg):
    for q in _moduli() + [0, 1, 4, 5, (1 << 44) + 1, 2**64 - 1]:
        h = q // 2
        for n in (2, 64, 256, 4096, 65536, 131072, 0, 3):
            assert pkg.ring_mod_capacity_product(q, n, h, h) == pkg.ring_mod_capacity(q, n), (q, n)
            for bound in (1, 128, h):
                assert pkg.ring_mod_capacity_product(q, n, h, bound) == pkg.ring_mod_capacity_bounded(q, n, bound) \
                    == pkg.ring_mod_capacity_product(q, n, bound, h), (q, n, bound)
            if pkg.ring_mod_capacity(q, n) == 0:
                assert pkg.ring_mod_capacity_product(q, n, 1, 1) == 0, (q, n)
    assert pkg.ring_mod_capacity_product(Q40, 64, 128, 128) == 2**64 - 1                       # saturated
    assert pkg.ring_mod_capacity_product(1 << 32, 4096, 128, 128) == 2305840781199673368
    assert pkg.ring_mod_capacity_product(Q40, 64, 0, 0) == 0 and pkg.ring_mod_capacity_product(Q40, 64, 1 << 37, Q40 // 2) == 31
    assert pkg.ring_mod_capacity(8246337208321, 8) == 1
    assert pkg.ring_mod_capacity_product(2**64, 64, 1, 1) == 0 and pkg.ring_mod_capacity_product(3329, 64, -1, 1) == 0     # the wrapper's range check


class Fake:
    """The library, buffers apart from each other and a ring handle of zeros with its leading fields settable."""

    def __init__(self, pkg):
        self.pkg, self.lib = pkg, pkg._abi.load_library()
        self.bufs = [(ctypes.c_uint64 * 1024)() for _ in range(4)]
        self.h_buf = (ctypes.c_uint64 * 512)()
        self.g, self.a, self.b, self.status = (ctypes.addressof(b) for b in self.bufs)
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
    sym2, device = "sym2" in name, name.endswith("device")

    def call(h, g, status, a, b, batch=1, ra=2, rb=2, width=2, bound_a=0, bound_b=0):
        args = [h, g, status, a, b, batch, ra] + ([] if sym2 else [rb]) + [width, bound_a, bound_b] + ([None] if device else [])
        return getattr(f.lib, name)(*args)

    def refused(word, *args, **kw):
        assert call(*args, **kw) == -1
        msg = f.message(name)
        assert word in msg, msg
        return msg

    f.ring(3329, 4)
    h = 3329 // 2
    # (1) NULL handle, g, status, a (sym2: b), whatever the shape
    for args in [(None, f.g, f.status, f.a, f.b), (f.h, None, f.status, f.a, f.b), (f.h, f.g, None, f.a, f.b), (f.h, f.g, f.status, None, f.b)] + \
            ([(f.h, f.g, f.status, f.a, None)] if sym2 else []):
        refused("NULL", *args)
        refused("NULL", *args, ra=0, width=MAX_TERMS + 1, bound_a=h + 1)
    # (2) zero shapes before the caps, (4) vectors before (5) width, before the bounds
    refused("at least 1", f.h, f.g, f.status, f.a, f.b, ra=0, rb=0, width=MAX_TERMS + 1)
    refused("at least 1", f.h, f.g, f.status, f.a, f.b, ra=MAX_VECTORS + 1, rb=MAX_VECTORS + 1, width=0)
    if not sym2:
        refused("rb == ra", f.h, f.g, f.status, f.a, None, ra=2, rb=3, width=MAX_TERMS + 1)     # (3)
    refused("LSR_RING_GRAM_MAX_VECTORS", f.h, f.g, f.status, f.a, f.b, ra=MAX_VECTORS + 1, rb=MAX_VECTORS + 1, width=MAX_TERMS + 1)
    refused("LSR_RING_DOT_MAX_TERMS", f.h, f.g, f.status, f.a, f.b, width=MAX_TERMS + 1, bound_a=h + 1)
    refused("overflow", f.h, f.g, f.status, f.a, f.b, batch=2**60, bound_a=h + 1)                # (6)
    # (7) a bound above floor(q / 2), before the empty call and before the overlap
    for kw in ({"bound_a": h + 1}, {"bound_b": h + 1}, {"bound_a": 2**64 - 1, "bound_b": 1}):
        msg = refused("above floor(q / 2)", f.h, f.g, f.status, f.a, f.b, batch=0, **kw)
        assert str(h) in msg
    refused("above floor(q / 2)", f.h, f.a, f.status, f.a, f.b, bound_a=h + 1)
    if not sym2:                                              # the symmetric form does not read bound_b
        assert call(f.h, f.g, f.status, f.a, None, batch=0, bound_a=h, bound_b=h + 1) == 0
    # (8) the empty call is a no-op
    assert call(f.h, f.a, f.status, f.a, f.b, batch=0, bound_a=h, bound_b=1) == 0
    # (9) family bytes before (10) the workspace
    f.ring(1 << 32, 4096)
    refused("LSR_RING_GRAM_MAX_FAMILY_BYTES", f.h, f.a, f.status, f.a, f.b, ra=64, rb=64, width=4096)
    # (10) a family that does not fit even one column at a time (n = 131072: 64 polynomials per prime), before the overlap
    f.ring(3329, 131072)
    msg = refused("one column at a time", f.h, f.a, f.status, f.a, f.b, ra=10, rb=10, width=1)
    assert "LAMBDA_SNARK_NTT_CHUNK_MIB" in msg
    # (11) sym2 where P carries one product, naming the cross form, before the overlap
    f.ring(8246337208321, 8)
    if sym2:
        msg = refused("lsr_ring_mod_gram_batch", f.h, f.a, f.status, f.a, f.b)
        assert "cross form" in msg
    # (12) overlaps: g and an operand, status and an operand, status and g — before the device
    refused("g overlaps a", f.h, f.a, f.status, f.a, f.b, bound_a=1 if sym2 else 0, bound_b=1 if sym2 else 0)
    refused("g overlaps b", f.h, f.b + 8, f.status, f.a, f.b, bound_a=1, bound_b=1)
    refused("status overlaps a", f.h, f.g, f.a + 64, f.a, f.b, bound_a=1, bound_b=1)
    refused("status overlaps g", f.h, f.g, f.g, f.a, f.b, bound_a=1, bound_b=1)


def test_prepare_refuses_a_null_handle(fake):
    assert fake.lib.lsr_ring_mod_gram_prepare(None) == -1
    assert "NULL" in fake.message("lsr_ring_mod_gram_prepare")
