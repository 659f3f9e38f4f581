"""CPU suite: the masked response with its abort under an arbitrary modulus (lsr_ring_mod_respond_batch, batch.h "responses under
any modulus") is declared, exported and mirrored in ctypes and in RingMod, and the refusals that need no device come
in batch.h's order, so they answer -1 with a message on a machine without a GPU.

The handle of the refusal tests is fake and never used as a handle: those refusals read only the leading fields LsrRingMod documents
(q, n; logn is the third), and every call made here is refused before any device work — also on a machine that has a GPU."""
import ctypes
import os
import re

import pytest

from ring_mod_respond_model import (test_model_response_is_the_fold_plus_the_mask,  # noqa: F401  (collected here: the model's own tests)
                                    test_model_statuses_and_their_precedence)  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_H = os.path.join(ROOT, "include", "lambda_snark", "batch.h")
ARGUMENTS = {
    "lsr_ring_mod_respond_batch": ["h", "out", "status", "y", "v", "p", "outputs", "terms", "term_stride", "width", "bound_y", "bound_v", "bound_p",
                                   "bound_z"],
    "lsr_ring_mod_respond_batch_device": ["h", "d_out", "d_status", "d_y", "d_v", "d_p", "outputs", "terms", "term_stride", "width", "bound_y", "bound_v",
                                          "bound_p", "bound_z", "stream"],
}
MAX_TERMS, MAX_WIDTH = 65536, 65536


def test_batch_h_declares_the_functions_in_their_section_with_the_contract():
    raw = open(BATCH_H).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, want in ARGUMENTS.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*LSR_NOEXCEPT", text)
        assert m, name
        assert [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")] == want, name
    # after the quadratic forms of the handle, before the Gaussian sampler
    assert text.index("lsr_ring_mod_quadform_batch_device") < text.index("lsr_ring_mod_respond_batch") \
        < text.index("lsr_ring_mod_respond_batch_device") < text.index("lsr_sample_gaussian_seeded")
    assert raw.index("NTT: quadratic forms under any modulus") < raw.index("NTT: responses under any modulus") < raw.index("Gaussian sampler: seeded / device")
    section = raw[raw.index("NTT: responses under any modulus"):raw.index("Gaussian sampler: seeded / device")]
    assert re.search(r"#define\s+LSR_RING_RESPOND_REJECTED\s+2\b", section)
    for status in (r"^ \*\s+-1   ", r"^ \*\s+0   ", r"^ \*\s+2   LSR_RING_RESPOND_REJECTED", r"^ \*\s+1   accepted"):
        assert re.search(status, section, flags=re.M), status       # the four statuses
    for word in ("z[j] = (f[j] + y[j]) mod q word for word", "-1 wins over 0, 0 wins over 2, 2 wins over 1", "EVERY word of out[j] is 0",
                 "y may be exactly out", "Any other overlap", "is refused", "LSR_RING_RESPOND_REJECTED", "0 for any of them states none",
                 "bound_z == 0 never rejects", "equals lsr_ring_mod_fold_batch word for word", "centred mod q",
                 "bound_y + terms n bound_v bound_p < q/2", "later group of terms", "later chunk of", "lsr_ring_mod_capacity_product(q, n, bound_v, bound_p)",
                 "n <= 4096", "names the composed route", "lsr_ntt_ring_linf_batch_device", "the message names all four", "there is no", "_prepare",
                 "LAMBDA_SNARK_STAGING_MIB", "not bracketed"):
        assert word in section, word                               # the definition is the contract and lives in the header


def test_library_exports_signatures_and_members(pkg):
    lib = pkg._abi.load_library()
    for name, want in ARGUMENTS.items():
        assert hasattr(lib, name), name
        result, arguments = pkg._abi.SIGNATURES[name]
        assert result is ctypes.c_int and len(arguments) == len(want), name
        sizes = [i for i, a in enumerate(want) if a in ("outputs", "terms", "term_stride", "width")]
        bounds = [i for i, a in enumerate(want) if a.startswith("bound_")]
        assert len(sizes) == 4 and len(bounds) == 4
        assert all(arguments[i] is ctypes.c_size_t for i in sizes) and all(arguments[i] is ctypes.c_uint64 for i in bounds), name
        assert all(arguments[i] is ctypes.c_void_p for i in range(len(want)) if i not in sizes + bounds), name
    for member in ("respond", "respond_device"):
        assert hasattr(pkg.RingMod, member), member
    assert pkg.RING_RESPOND_REJECTED == 2 and "RING_RESPOND_REJECTED" in pkg.__all__


class Fake:
    """The library, buffers apart from each other and a ring handle of zeros with its leading fields settable."""

    def __init__(self, pkg):
        self.pkg, self.lib = pkg, pkg._abi.load_library()
        self.bufs = [(ctypes.c_uint64 * 1024)() for _ in range(5)]
        self.h_buf = (ctypes.c_uint64 * 512)()
        self.out, self.y, self.v, self.p, self.status = (ctypes.addressof(b) for b in self.bufs)
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

    def call(h, out, status, y, v, p, outputs=2, terms=2, term_stride=2, width=2, bound_y=0, bound_v=0, bound_p=0, bound_z=0):
        args = [h, out, status, y, v, p, outputs, terms, term_stride, width, bound_y, bound_v, bound_p, bound_z] + ([None] if device else [])
        return getattr(f.lib, name)(*args)

    def refused(word, *args, **kw):
        assert call(*args, **kw) == -1
        msg = f.message(name)
        assert word in msg, msg
        return msg

    f.ring(3329, 4)
    h = 3329 // 2
    good = (f.h, f.out, f.status, f.y, f.v, f.p)
    # (1) NULL handle, out, status, v or p, whatever the shape — y may be NULL
    for i in (0, 1, 2, 4, 5):
        args = list(good)
        args[i] = None
        refused("NULL", *args)
        refused("NULL", *args, terms=0, width=MAX_WIDTH + 1, bound_z=h + 1)
    # (2) terms == 0 before (3) the empty call, which comes before every cap and before the bounds
    refused("at least 1", *good, terms=0, outputs=0)
    refused("at least 1", *good, terms=0, width=0)
    for kw in ({"outputs": 0}, {"width": 0}):
        assert call(*good, terms=MAX_TERMS + 1, bound_z=h + 1, **kw) == 0
        assert call(f.h, f.v, f.status, None, f.v, f.p, bound_y=1, **kw) == 0     # (an overlap and a bound nobody looks at)
    # (4) terms before (5) width before (6) the sizes before (7) the bounds
    refused("LSR_RING_DOT_MAX_TERMS", *good, terms=MAX_TERMS + 1, width=MAX_WIDTH + 1, bound_z=h + 1)
    refused("LSR_RING_FOLD_MAX_WIDTH", *good, width=MAX_WIDTH + 1, outputs=2**60, bound_y=h + 1)
    refused("overflow", *good, outputs=2**60, bound_z=h + 1)
    refused("overflow", *good, outputs=3, term_stride=2**63, bound_p=h + 1)
    # (7) a NULL y with a bound on it, then a bound above floor(q / 2): all four bounds by name, before (8) the range of n
    msg = refused("y is NULL", f.h, f.out, f.status, None, f.v, f.p, bound_y=1, bound_z=h + 1)
    assert all(word in msg for word in ("bound_y = 1", "bound_v = 0", "bound_p = 0", "bound_z = %d" % (h + 1)))
    for kw in ({"bound_y": h + 1}, {"bound_v": h + 1}, {"bound_p": h + 1}, {"bound_z": h + 1}, {"bound_z": 2**64 - 1, "bound_p": 1}):
        msg = refused("above floor(q / 2)", *good, **kw)
        assert str(h) in msg and all(word in msg for word in ("bound_y = ", "bound_v = ", "bound_p = ", "bound_z = "))
    f.ring(3329, 8192)
    refused("above floor(q / 2)", *good, bound_z=h + 1)
    refused("y is NULL", f.h, f.out, f.status, None, f.v, f.p, bound_y=h)
    # (8) n above 4096: the composed route by name, before (10) the overlaps
    msg = refused("above 4096", f.h, f.v, f.status, f.y, f.v, f.p, bound_y=h, bound_v=h, bound_p=1, bound_z=h)
    for word in ("lsr_ring_mod_lift_batch_device", "lsr_ntt_ring_fold_batch_device", "lsr_ring_mod_prime_context", "lsr_ring_mod_reduce_batch_device",
                 "max_terms", "accumulate", "add y mod q", "lsr_ntt_ring_linf_batch_device", "lsr_ring_mod_coeff_context"):
        assert word in msg, word
    # (9) byte sizes at the handle's n: 2^50 polynomials pass (6) at 16 bytes each and overflow at n = 4096
    f.ring(3329, 4096)
    refused("overflow size_t at this ring degree", *good, outputs=2**34, terms=1, term_stride=0, width=2**16)
    # (10) overlaps: out and an operand, status and an operand, status and out — before the device
    f.ring(3329, 4)
    refused("out overlaps y", f.h, f.out, f.status, f.out + 8, f.v, f.p)                      # one word off: not in place
    refused("out overlaps y", f.h, f.out + 2 * 2 * 4 * 8 - 8, f.status, f.out, f.v, f.p)       # the last word of y, the first of out
    refused("out overlaps v", f.h, f.v, f.status, f.y, f.v, f.p)
    refused("out overlaps p", f.h, f.p + 8, f.status, None, f.v, f.p, bound_v=1, bound_p=1, bound_z=1)
    refused("status overlaps y", f.h, f.out, f.y + 64, f.y, f.v, f.p)
    refused("status overlaps v", f.h, f.out, f.v + 64, f.y, f.v, f.p)
    refused("status overlaps p", f.h, f.out, f.p, f.y, f.v, f.p)
    refused("status overlaps out", f.h, f.out, f.out + 8, f.y, f.v, f.p)
    # y == out is the in-place form and passes the first of these: the next refusal in the order ends the call before any device work
    refused("out overlaps v", f.h, f.v, f.status, f.v, f.v, f.p)
    refused("status overlaps v", f.h, f.out, f.v, f.out, f.v, f.p, bound_y=h)
    refused("status overlaps out", f.h, f.out, f.out + 8, f.out, f.v, f.p)
