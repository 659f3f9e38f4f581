"""CPU suite: the bit-packed ring elements (lsr_ring_pack_words, lsr_ring_pack_min_bits, lsr_ntt_ring_pack_batch,
lsr_ntt_ring_unpack_batch and the _device forms) are declared, exported and mirrored in ctypes, the Python members exist
on both context classes, the two host-only functions agree with the model, and the refusals come before any device work, in
batch.h's order — so they answer -1 with a message on a machine without a GPU.

The handle is fake and never used as one: the refusals read nothing of a context but its degree, the second field of the handle
(lsr_runtime.hpp), which the fake sets."""
import ctypes
import os
import re

import pytest

import ring_pack_model as model
from ring_pack_model import (test_by_hand_vector_packs_to_0x8f9,  # noqa: F401  (collected here: the model's own tests)
                             test_round_trips_with_the_end_values,  # noqa: F401
                             test_the_three_invalid_decodes,  # noqa: F401
                             test_words_and_min_bits)  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_H = os.path.join(ROOT, "include", "lambda_snark", "batch.h")
PACK, UNPACK = "lsr_ntt_ring_pack_batch", "lsr_ntt_ring_unpack_batch"
ARGUMENTS = {
    "lsr_ring_pack_words": ["n", "bits"],
    "lsr_ring_pack_min_bits": ["q", "mode", "bound"],
    PACK: ["ctx", "out", "status", "x", "count", "mode", "bits"],
    PACK + "_device": ["ctx", "d_out", "d_status", "d_x", "count", "mode", "bits", "stream"],
    UNPACK: ["ctx", "out", "status", "in", "count", "mode", "bits"],
    UNPACK + "_device": ["ctx", "d_out", "d_status", "d_in", "count", "mode", "bits", "stream"],
}
MEMBERS = ("ring_pack", "ring_pack_device", "ring_unpack", "ring_unpack_device")
ENTRIES = [(PACK, False), (PACK + "_device", True), (UNPACK, False), (UNPACK + "_device", True)]


class Fake:
    """The library, three buffers apart from each other, and a context of zeros but for its modulus and degree."""

    def __init__(self, pkg, q=model.Q44, n=64):
        self.pkg, self.lib = pkg, pkg._abi.load_library()
        self.bufs = [(ctypes.c_uint64 * 16)() for _ in range(3)]
        self.ctx_buf = (ctypes.c_uint64 * 128)()
        self.a, self.b, self.c = (ctypes.addressof(b) for b in self.bufs)
        self.ctx = ctypes.addressof(self.ctx_buf)
        self.ctx_buf[0], self.ctx_buf[1] = q, n              # uint64 modulus; uint32 degree

    def call(self, name, device, ctx, out, status, src, count=1, mode=0, bits=11):
        f = getattr(self.lib, name)
        return f(ctx, out, status, src, count, mode, bits, None) if device else f(ctx, out, status, src, count, mode, bits)

    def refused(self, name, device, word, *others, **kw):
        assert self.call(name, device, self.ctx, self.a, self.b, self.c, **kw) == -1, kw
        msg = self.pkg._abi.last_error()
        assert msg.startswith(name + ":") and word in msg, (kw, msg)
        for other in others:
            assert other not in msg, (kw, msg)


@pytest.fixture()
def fake(pkg):
    return Fake(pkg)


def test_batch_h_declares_the_functions_with_their_argument_names_and_the_definition():
    raw = open(BATCH_H).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, want in ARGUMENTS.items():
        m = re.search(r"\b(?:int|size_t|unsigned)\s+" + name + r"\s*\(([^)]*)\)\s*LSR_NOEXCEPT", text)
        assert m, name
        assert [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")] == want, name
    assert text.index("lsr_ntt_ring_challenge_batch_device") < text.index("lsr_ring_pack_words") < text.index("lsr_sample_gaussian_seeded")
    for word in ("LSR_RING_PACK_CENTRED", "LSR_RING_PACK_RESIDUE", "Bit b of field i is bit i*bits + b", "Stream bit t is bit t mod 64 of word floor(t/64)",
                 "W = ceil(n*bits/64)", "This outranks everything", "An invalid field writes the word 0", "A non-zero padding bit makes the status 0",
                 "unique preimage", "Every word of `out` is below q", "bitlen(bound) + 1"):
        assert word in raw, word                               # the definition is the contract and lives in the header


def test_library_exports_signatures_members_and_constants(pkg):
    lib = pkg._abi.load_library()
    for name, want in ARGUMENTS.items():
        assert hasattr(lib, name), name
        assert len(pkg._abi.SIGNATURES[name][1]) == len(want), name
    for cls in (pkg.NttContext, pkg.CyclicNtt):
        assert issubclass(cls, pkg._RingPack)
        for member in MEMBERS:
            assert callable(getattr(cls, member)), member
    text = open(BATCH_H).read()
    for macro, mirror, want in [("LSR_RING_PACK_CENTRED", "RING_PACK_CENTRED", model.CENTRED), ("LSR_RING_PACK_RESIDUE", "RING_PACK_RESIDUE", model.RESIDUE)]:
        assert int(re.search(r"#define\s+" + macro + r"\s+(\d+)", text).group(1)) == getattr(pkg, mirror) == want, macro
        assert mirror in pkg.__all__
    assert "ring_pack_words" in pkg.__all__ and "ring_pack_min_bits" in pkg.__all__


def test_words_and_min_bits_are_the_models(pkg):
    for n in [2, 4, 16, 32, 64, 128, 4096, 1 << 16, 1 << 22]:
        for bits in range(0, 66):
            assert pkg.ring_pack_words(n, bits) == model.words(n, bits), (n, bits)
    assert pkg.ring_pack_words(64, 2**32 - 1) == 0 and pkg.ring_pack_words(64, 2**32 + 11) == 0
    bounds = [0, 1, 2, 3, 4, 1023, 1024, 2**31 - 1, 2**31, 2**43, 2**61, 2**62 - 1, 2**62, 2**63 - 1, 2**63, 2**64 - 1]
    for q in [3, 12289, model.Q44, 1152921504606584833, model.GOLDILOCKS]:
        for bound in bounds + [(q - 1) // 2 - 1, (q - 1) // 2, (q - 1) // 2 + 1, q - 2, q - 1, q]:
            for mode in (model.CENTRED, model.RESIDUE, 2, -1):
                assert pkg.ring_pack_min_bits(q, mode, bound) == model.min_bits(q, mode, bound), (q, mode, bound)
    # the gadget's digit range is the field's: digits of base 2^b pack at b bits, BALL and ternary elements at 2
    assert pkg.ring_pack_min_bits(model.Q44, model.CENTRED, 1) == 2
    assert pkg.ring_pack_min_bits(model.Q44, model.CENTRED, 1 << 10) == 12 and pkg.ring_pack_min_bits(model.Q44, model.CENTRED, (1 << 10) - 1) == 11


@pytest.mark.parametrize("name,device", ENTRIES)
def test_refusals_in_the_documented_order(pkg, fake, name, device):
    f = fake
    # (1) NULL, before everything that follows (each of which would refuse too) and before the empty call
    for ctx, out, status, src in [(None, f.a, f.b, f.c), (f.ctx, None, f.b, f.c), (f.ctx, f.a, None, f.c), (f.ctx, f.a, f.b, None)]:
        for kw in [{}, dict(count=0), dict(mode=2), dict(bits=0), dict(bits=64, mode=-1, count=2**64 - 1)]:
            assert f.call(name, device, ctx, out, status, src, **kw) == -1
            msg = pkg._abi.last_error()
            assert msg.startswith(name + ":") and "NULL" in msg, msg
    # (2) the mode, then bits, before the empty call and the overflowing size
    for mode in (2, -1, 7):
        for kw in [{}, dict(count=0), dict(bits=0), dict(bits=64), dict(count=2**64 - 1)]:
            f.refused(name, device, "mode", "bits =", "overflow", mode=mode, **kw)
    for bits in (0, 64, 65, 2**32 - 1):
        for kw in [{}, dict(count=0), dict(mode=1), dict(count=2**64 - 1)]:
            f.refused(name, device, "bits", "overflow", bits=bits, **kw)
    # (3) the empty call is a no-op, whatever overlaps
    for mode in (0, 1):
        for bits in (1, 11, 63):
            assert f.call(name, device, f.ctx, f.a, f.a, f.a, count=0, mode=mode, bits=bits) == 0
    # (4) the sizes
    for count, bits in [(2**64 - 1, 11), (2**58, 1), (2**61, 63), (2**55, 63)]:
        f.refused(name, device, "overflow", count=count, bits=bits)


def test_python_wrappers_check_the_shapes(pkg):
    class Ctx(pkg._RingPack):
        n, _h, _lib = 16, None, None
    import numpy as np
    with pytest.raises(ValueError, match=r"\[n\]"):
        Ctx().ring_pack(np.zeros(15, dtype=np.uint64), 3)
    with pytest.raises(ValueError, match="ring_pack_words"):
        Ctx().ring_unpack(np.zeros(2, dtype=np.uint64), 3)
