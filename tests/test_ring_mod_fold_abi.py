"""CPU suite: the fold of ring vectors by challenges under an arbitrary modulus (lsr_ring_mod_fold_batch, batch.h "fold under any
modulus") is declared, exported and mirrored in ctypes and in RingMod, and the refusals that need no device come in
batch.h's order, so they answer -1 with a message on a machine without a GPU.

The handle of the refusal tests is fake and never used as a handle: those refusals read only the leading fields LsrRingMod documents
(q, n; logn is the third), and every call made here is refused before any device work — also on a machine that has a GPU."""
import ctypes
import os
import re

import pytest

from ring_mod_fold_model import (test_model_fold_is_the_schoolbook_at_every_stride,  # noqa: F401  (collected here: the model's own tests)
                                 test_model_status_gates_and_groups)  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_H = os.path.join(ROOT, "include", "lambda_snark", "batch.h")
ARGUMENTS = {
    "lsr_ring_mod_fold_batch": ["h", "out", "status", "v", "p", "outputs", "terms", "term_stride", "width", "bound_v", "bound_p"],
    "lsr_ring_mod_fold_batch_device": ["h", "d_out", "d_status", "d_v", "d_p", "outputs", "terms", "term_stride", "width", "bound_v", "bound_p", "stream"],
}
MAX_TERMS, MAX_WIDTH = 65536, 65536


def test_batch_h_declares_the_functions_in_their_section_with_the_contract():
    raw = open(BATCH_H).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, want in ARGUMENTS.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*LSR_NOEXCEPT", text)
        assert m, name
        assert [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")] == want, name
    # after the Gram matrices of the handle, before the Gaussian sampler
    assert text.index("lsr_ring_mod_gram_sym2_batch_device") < text.index("lsr_ring_mod_fold_batch") \
        < text.index("lsr_ring_mod_fold_batch_device") < text.index("lsr_sample_gaussian_seeded")
    section = raw[raw.index("NTT: fold under any modulus"):raw.index("Gaussian sampler: seeded / device")]
    assert raw.index("NTT: Gram matrices under any modulus") < raw.index("NTT: fold under any modulus")
    for word in ("lsr_ring_mod_dot_batch on the gathered operands", "word for word", "-1 wins over 0", "EVERY word of out[j] is 0", "0 states none",
                 "gates every output", "gates output j alone", "lsr_ring_mod_capacity_product(q, n, bound_v, bound_p)",
                 "Exactness never depends on the caller knowing a capacity", "2199021131876", "n <= 4096", "names the composed route",
                 "lsr_ring_mod_create allocates it", "there is no _prepare", "LAMBDA_SNARK_STAGING_MIB", "not bracketed"):
        assert word in section, word                               # the definition is the contract and lives in the header
    composition = raw[raw.index("Composition.  Together with"):raw.index("The fused calls, n <= 4096:")]
    assert "lsr_ntt_ring_fold_batch" in composition               # still composable, and the only route above n = 4096


def test_library_exports_signatures_and_members(pkg):
    lib = pkg._abi.load_library()
    for name, want in ARGUMENTS.items():
        assert hasattr(lib, name), name
        result, arguments = pkg._abi.SIGNATURES[name]
        assert result is ctypes.c_int and len(arguments) == len(want), name
        sizes = [i for i, a in enumerate(want) if a in ("outputs", "terms", "term_stride", "width")]
        bounds = [i for i, a in enumerate(want) if a.startswith("bound_")]
        assert all(arguments[i] is ctypes.c_size_t for i in sizes) and all(arguments[i] is ctypes.c_uint64 for i in bounds), name
        assert all(arguments[i] is ctypes.c_void_p for i in range(len(want)) if i not in sizes + bounds), name
    for member in ("fold", "fold_device"):
        assert hasattr(pkg.RingMod, member), member


class Fake:
    """The library, buffers apart from each other and a ring handle of zeros with its leading fields settable."""

    def __init__(self, pkg):
        self.pkg, self.lib = pkg, pkg._abi.load_library()
        self.bufs = [(ctypes.c_uint64 * 1024)() for _ in range(4)]
        self.h_buf = (ctypes.c_uint64 * 512)()
        self.out, self.v, self.p, self.status = (ctypes.addressof(b) for b in self.bufs)
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


@pytest.mark.parametrize("name", list(ARGUMENTS))
def test_refusals_without_a_device_in_the_documented_order(fake, name):
    f = fake
    device = name.endswith("device")

    def call(h, out, status, v, p, outputs=2, terms=2, term_stride=2, width=2, bound_v=0, bound_p=0):
        args = [h, out, status, v, p, outputs, terms, term_stride, width, bound_v, bound_p] + ([None] if device else [])
        return getattr(f.lib, name)(*args)

    def refused(word, *args, **kw):
        assert call(*args, **kw) == -1
        msg = f.message(name)
        assert word in msg, msg
        return msg

    f.ring(3329, 4)
    h = 3329 // 2
    good = (f.h, f.out, f.status, f.v, f.p)
    # (1) NULL handle, out, status, v or p, whatever the shape
    for i in range(5):
        args = list(good)
        args[i] = None
        refused("NULL", *args)
        refused("NULL", *args, terms=0, width=MAX_WIDTH + 1, bound_v=h + 1)
    # (2) terms == 0 before (3) the empty call, which comes before every cap and before the bounds
    refused("at least 1", *good, terms=0, outputs=0)
    refused("at least 1", *good, terms=0, width=0)
    for kw in ({"outputs": 0}, {"width": 0}):
        assert call(*good, terms=MAX_TERMS + 1, bound_v=h + 1, **kw) == 0
        assert call(f.h, f.v, f.status, f.v, f.p, **kw) == 0              # (an overlap nobody looks at)
    # (4) terms before (5) width before (6) the sizes before (7) the bounds
    refused("LSR_RING_DOT_MAX_TERMS", *good, terms=MAX_TERMS + 1, width=MAX_WIDTH + 1, bound_v=h + 1)
    refused("LSR_RING_FOLD_MAX_WIDTH", *good, width=MAX_WIDTH + 1, outputs=2**60, bound_v=h + 1)
    refused("overflow", *good, outputs=2**60, bound_v=h + 1)
    refused("overflow", *good, outputs=3, term_stride=2**63, bound_p=h + 1)
    # (7) a bound above floor(q / 2), before (8) the range of n
    for kw in ({"bound_v": h + 1}, {"bound_p": h + 1}, {"bound_v": 2**64 - 1, "bound_p": 1}):
        msg = refused("above floor(q / 2)", *good, **kw)
        assert str(h) in msg
    f.ring(3329, 8192)
    refused("above floor(q / 2)", *good, bound_p=h + 1)
    # (8) n above 4096: the composed route by name, before (10) the overlaps
    msg = refused("above 4096", f.h, f.v, f.status, f.v, f.p, bound_v=h, bound_p=1)
    for word in ("lsr_ring_mod_lift_batch_device", "lsr_ntt_ring_fold_batch_device", "lsr_ring_mod_prime_context", "lsr_ring_mod_reduce_batch_device",
                 "max_terms", "accumulate"):
        assert word in msg, word
    # (9) byte sizes at the handle's n: 2^50 polynomials pass (6) at 16 bytes each and overflow at n = 4096
    f.ring(3329, 4096)
    refused("overflow size_t at this ring degree", *good, outputs=2**34, terms=1, term_stride=0, width=2**16)
    # (10) overlaps: out and an operand, status and an operand, status and out — before the device
    f.ring(3329, 4)
    refused("out overlaps v", f.h, f.v, f.status, f.v, f.p)
    refused("out overlaps p", f.h, f.p + 8, f.status, f.v, f.p, bound_v=1, bound_p=1)
    refused("status overlaps v", f.h, f.out, f.v + 64, f.v, f.p)
    refused("status overlaps p", f.h, f.out, f.p, f.v, f.p)
    refused("status overlaps out", f.h, f.out, f.out + 8, f.v, f.p)
