"""CPU suite: the ring handles under an arbitrary modulus (lsr_ring_mod_*, batch.h "ring products under any modulus")
are declared, exported and mirrored in ctypes and in the RingMod class; the two host-only functions (the prime pair and the
capacity) agree with the Python-integer model (tests/ring_mod_model.py) and with the RNS commitment contexts' moduli; and the
refusals that need no device come in batch.h's order, so they answer -1 with a message on a machine without a GPU.

The handle of the refusal tests is fake and never used as one: those refusals read nothing of a handle."""
import ctypes
import os
import re

import pytest

import ring_mod_model as model
from ring_mod_model import (test_kronecker_equals_schoolbook,  # noqa: F401  (collected here: the model's own tests)
                            test_lift_and_reduce_round_trip,  # noqa: F401
                            test_planted_arrays_hold_the_five_edge_words,  # noqa: F401
                            test_planted_products_tell_broken_lift_and_reduce_apart,  # noqa: F401
                            test_primes_follow_the_rule)  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_H = os.path.join(ROOT, "include", "lambda_snark", "batch.h")
ARGUMENTS = {
    "lsr_ring_mod_create": ["q", "n", "device"],
    "lsr_ring_mod_free": ["h"],
    "lsr_ring_mod_modulus": ["h"],
    "lsr_ring_mod_prime_context": ["h", "i"],
    "lsr_ring_mod_max_terms": ["h"],
    "lsr_ring_mod_primes": ["n", "primes[2]"],
    "lsr_ring_mod_capacity": ["q", "n"],
    "lsr_ring_mod_lift_batch_device": ["h", "i", "d_out", "d_x", "count", "stream"],
    "lsr_ring_mod_reduce_batch_device": ["h", "d_out", "d_r0", "d_r1", "count", "accumulate", "stream"],
    "lsr_ring_mod_mul_batch": ["h", "c", "a", "b", "batch", "b_rows"],
    "lsr_ring_mod_mul_batch_device": ["h", "d_c", "d_a", "d_b", "batch", "b_rows", "stream"],
    "lsr_ring_mod_dot_batch": ["h", "c", "a", "b", "batch", "terms", "b_rows"],
    "lsr_ring_mod_dot_batch_device": ["h", "d_c", "d_a", "d_b", "batch", "terms", "b_rows", "stream"],
}
MEMBERS = ("primes", "max_terms", "prime_context", "lift_device", "reduce_device", "mul", "mul_device", "dot", "dot_device", "close")


def test_batch_h_declares_the_functions_in_their_section_with_the_contract():
    raw = open(BATCH_H).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, want in ARGUMENTS.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*LSR_NOEXCEPT", text)
        assert m, name
        assert [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")] == want, name
    assert "typedef struct LsrRingMod LsrRingMod;" in text
    # after the bit-packing section, before the Gaussian sampler
    assert text.index("lsr_ntt_ring_unpack_batch_device") < text.index("typedef struct LsrRingMod") < text.index("lsr_ring_mod_dot_batch_device") \
        < text.index("lsr_sample_gaussian_seeded")
    for word in ("max_terms = floor(((P - 1)/2) / (n h^2))", "must not exceed max_terms", "lsr_ntt_ring_fold_batch", "lsr_ntt_ring_matvec_batch",
                 "lsr_ntt_ring_gram_batch", "lsr_ntt_ring_gram_sym2_batch", "lsr_ntt_ring_dot_galois_batch", "[-(P-1)/2, (P-1)/2]",
                 "d_out may be d_x itself", "from the first call"):
        assert word in raw, word                               # the definition is the contract and lives in the header


def test_library_exports_signatures_and_members(pkg):
    lib = pkg._abi.load_library()
    for name, want in ARGUMENTS.items():
        assert hasattr(lib, name), name
        assert len(pkg._abi.SIGNATURES[name][1]) == len(want), name
    assert pkg._abi.SIGNATURES["lsr_ring_mod_create"][0] is ctypes.c_void_p and pkg._abi.SIGNATURES["lsr_ring_mod_prime_context"][0] is ctypes.c_void_p
    assert pkg._abi.SIGNATURES["lsr_ring_mod_capacity"][0] is ctypes.c_size_t and pkg._abi.SIGNATURES["lsr_ring_mod_modulus"][0] is ctypes.c_uint64
    for member in MEMBERS:
        assert hasattr(pkg.RingMod, member), member
    for name in ("RingMod", "ring_mod_primes", "ring_mod_capacity"):
        assert name in pkg.__all__


@pytest.mark.parametrize("n", [2, 64, 256, 4096, 65536])
def test_primes_are_the_models_and_the_rns_commitments(pkg, n):
    assert pkg.ring_mod_primes(n) == model.primes(n) == pkg.rns_commit_moduli(n)


def test_primes_refuse_other_degrees(pkg):
    lib = pkg._abi.load_library()
    out = (ctypes.c_uint64 * 2)()
    for n in (0, 1, 3, 96, 1 << 18, 2**32 - 1):
        assert model.primes(n) is None and lib.lsr_ring_mod_primes(n, out) == -1, n
    assert lib.lsr_ring_mod_primes(64, None) == -1


def test_capacity_is_the_models(pkg):
    p5 = model.prime_5_mod_8_below(1 << 32)
    assert p5 % 8 == 5 and model.is_prime(p5) and p5 > (1 << 32) - 1000
    top = model.largest_admissible(64)
    grid = [2, 3, 3329, 1 << 23, 1 << 32, p5, (1 << 40) + 15, top, top + 1]
    for n in (2, 64, 256, 4096, 65536, 131072):
        for q in grid + [0, 1, 4, 5, (1 << 44) - 1, 1 << 44, (1 << 44) + 1, 1 << 45, 1 << 63, 2**64 - 1, model.largest_admissible(n), model.largest_admissible(n) + 1]:
            assert pkg.ring_mod_capacity(q, n) == model.capacity(q, n), (q, n)
    assert pkg.ring_mod_capacity(top, 64) >= 1 and pkg.ring_mod_capacity(top + 1, 64) == 0
    assert pkg.ring_mod_capacity(2, 64) == 2**64 - 1 == pkg.ring_mod_capacity(3, 64)         # h = 1: saturated
    for n in (0, 1, 3, 1 << 18):
        assert pkg.ring_mod_capacity(3329, n) == 0
    # admissibility implies floor(q / 2) < 2^43 < p_i
    for n in (2, 64, 131072):
        assert model.largest_admissible(n) // 2 < 1 << 43 < min(model.primes(n))


def test_create_refuses_inadmissible_parameters_before_any_device_work(pkg):
    lib = pkg._abi.load_library()
    top = model.largest_admissible(64)
    for q, n, word in [(0, 64, "at least 2"), (1, 64, "at least 2"), (3329, 96, "power of two"), (3329, 1 << 18, "power of two"), (3329, 0, "power of two"),
                       (top + 1, 64, "too large"), (2**64 - 1, 2, "too large")]:
        assert not lib.lsr_ring_mod_create(q, n, 0), (q, n)
        msg = pkg._abi.last_error()
        assert msg.startswith("lsr_ring_mod_create:") and word in msg, msg
        with pytest.raises(pkg.CoreError):
            pkg.RingMod(q, n, device=0)
    lib.lsr_ring_mod_free(None)
    assert lib.lsr_ring_mod_modulus(None) == 0 and lib.lsr_ring_mod_max_terms(None) == 0
    assert not lib.lsr_ring_mod_prime_context(None, 0)


class Fake:
    """The library, three buffers apart from each other and a handle of zeros."""

    def __init__(self, pkg):
        self.pkg, self.lib = pkg, pkg._abi.load_library()
        self.bufs = [(ctypes.c_uint64 * 16)() for _ in range(3)]
        self.h_buf = (ctypes.c_uint64 * 256)()
        self.a, self.b, self.c = (ctypes.addressof(b) for b in self.bufs)
        self.h = ctypes.addressof(self.h_buf)

    def message(self, name):
        msg = self.pkg._abi.last_error()
        assert msg.startswith(name + ":"), msg
        return msg


@pytest.fixture()
def fake(pkg):
    return Fake(pkg)


@pytest.mark.parametrize("name,device,has_terms", [("lsr_ring_mod_mul_batch", False, False), ("lsr_ring_mod_mul_batch_device", True, False),
                                                   ("lsr_ring_mod_dot_batch", False, True), ("lsr_ring_mod_dot_batch_device", True, True)])
def test_product_refusals_in_the_documented_order(fake, name, device, has_terms):
    f = fake

    def call(h, c, a, b, batch=1, terms=1, b_rows=1):
        args = [h, c, a, b, batch] + ([terms] if has_terms else []) + [b_rows] + ([None] if device else [])
        return getattr(f.lib, name)(*args)

    # (1) NULL, before everything that follows (each of which would refuse too) and before the empty call
    for h, c, a, b in [(None, f.c, f.a, f.b), (f.h, None, f.a, f.b), (f.h, f.c, None, f.b), (f.h, f.c, f.a, None)]:
        for kw in [{}, dict(batch=0), dict(batch=5, b_rows=3), dict(terms=0), dict(terms=0, b_rows=7, batch=0)]:
            assert call(h, c, a, b, **kw) == -1
            assert "NULL" in f.message(name)
    # (2) b_rows, before terms and before the empty call
    for kw in [dict(batch=5, b_rows=3), dict(batch=0, b_rows=2), dict(batch=5, b_rows=0, terms=0), dict(batch=2, b_rows=3, terms=0)]:
        assert call(f.h, f.c, f.a, f.b, **kw) == -1
        msg = f.message(name)
        assert "b_rows" in msg and "terms must" not in msg, msg
    # (3) terms == 0, before the empty call
    if has_terms:
        for kw in [dict(terms=0), dict(terms=0, batch=0, b_rows=0), dict(terms=0, batch=4, b_rows=4)]:
            assert call(f.h, f.c, f.a, f.b, **kw) == -1
            assert "terms must be at least 1" in f.message(name)
    # (4) the empty call is a no-op, whatever overlaps
    assert call(f.h, f.a, f.a, f.a, batch=0, b_rows=0) == 0


def test_streaming_refusals_in_the_documented_order(fake):
    f = fake
    lift, reduce = f.lib.lsr_ring_mod_lift_batch_device, f.lib.lsr_ring_mod_reduce_batch_device
    for h, out, x in [(None, f.a, f.b), (f.h, None, f.b), (f.h, f.a, None)]:
        for i, count in [(0, 1), (2, 1), (-1, 0), (0, 0), (7, 2**64 - 1)]:
            assert lift(h, i, out, x, count, None) == -1
            assert "NULL" in f.message("lsr_ring_mod_lift_batch_device")
    for i in (2, -1, 7):
        for count in (1, 0, 2**64 - 1):                         # i before the empty call and the overflowing size
            assert lift(f.h, i, f.a, f.b, count, None) == -1
            msg = f.message("lsr_ring_mod_lift_batch_device")
            assert "must be 0 or 1" in msg and "overflow" not in msg, msg
    for i in (0, 1):
        assert lift(f.h, i, f.a, f.a, 0, None) == 0
        assert lift(f.h, i, f.a, f.b, 2**61, None) == -1
        assert "overflow" in f.message("lsr_ring_mod_lift_batch_device")
    for h, out, r0, r1 in [(None, f.a, f.b, f.c), (f.h, None, f.b, f.c), (f.h, f.a, None, f.c), (f.h, f.a, f.b, None)]:
        for count in (1, 0, 2**64 - 1):
            assert reduce(h, out, r0, r1, count, 0, None) == -1
            assert "NULL" in f.message("lsr_ring_mod_reduce_batch_device")
    assert reduce(f.h, f.a, f.b, f.c, 0, 1, None) == 0
    assert reduce(f.h, f.a, f.b, f.c, 2**61, 0, None) == -1
    assert "overflow" in f.message("lsr_ring_mod_reduce_batch_device")
    assert not f.lib.lsr_ring_mod_prime_context(f.h, 2) and not f.lib.lsr_ring_mod_prime_context(f.h, -1)
    assert f.lib.lsr_ring_mod_modulus(f.h) == 0


def test_python_wrappers_check_the_shapes(pkg):
    import numpy as np
    ring = pkg.RingMod.__new__(pkg.RingMod)
    ring.n, ring._h, ring._lib = 16, None, None
    with pytest.raises(ValueError, match="terms, n"):
        ring.dot(np.zeros(16, dtype=np.uint64), np.zeros(16, dtype=np.uint64))
    with pytest.raises(ValueError, match="at least 1"):
        ring.dot(np.zeros((0, 16), dtype=np.uint64), np.zeros((0, 16), dtype=np.uint64))
    with pytest.raises(ValueError, match="0 or 1"):
        ring.prime_context(2)
    assert pkg.ring_mod_capacity(2**64, 64) == 0 and pkg.ring_mod_capacity(-1, 64) == 0
