"""CPU suite: the fixed-point operator norm and the challenge sampler (lsr_ring_opnorm_table, lsr_ntt_ring_opnorm_prepare,
lsr_ntt_ring_opnorm_batch, lsr_ntt_ring_challenge_batch and the _device forms) are declared, exported and mirrored in
ctypes, the Python members exist on both context classes, the host-only cosine table is the documented one at every degree, and
every refusal comes before any device work, in batch.h's order — so it answers -1 with a message on a machine without a GPU.

The handle is fake and never used as one: the refusals read nothing of a context but its modulus and its degree, the first two fields
of the handle (lsr_runtime.hpp), which the fake sets."""
import ctypes
import os
import re

import numpy as np
import pytest

import ring_challenge_model as model
from ring_challenge_model import (test_cyclic_all_ones_has_norm_n_reached_at_e_zero,  # noqa: F401  (collected here: the model's own tests)
                                  test_norm_agrees_with_the_fft_norm_on_random_inputs,  # noqa: F401
                                  test_norm_of_a_monomial_is_one_within_the_documented_error,  # noqa: F401
                                  test_norm_of_one_is_exactly_one,  # noqa: F401
                                  test_out_of_range_elements_are_all_ones)  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_H = os.path.join(ROOT, "include", "lambda_snark", "batch.h")
TABLE, PREPARE, NORM, CHALLENGE = "lsr_ring_opnorm_table", "lsr_ntt_ring_opnorm_prepare", "lsr_ntt_ring_opnorm_batch", "lsr_ntt_ring_challenge_batch"
_SAMPLER = ["count", "kappa1", "kappa2", "opnorm_bound", "max_tries"]
ARGUMENTS = {
    TABLE: ["n", "out"],
    PREPARE: ["ctx"],
    NORM: ["ctx", "x", "count", "out"],
    NORM + "_device": ["ctx", "d_x", "count", "d_out", "stream"],
    CHALLENGE: ["ctx", "out", "tries"] + _SAMPLER + ["keys", "components", "domain", "index_base"],
    CHALLENGE + "_device": ["ctx", "d_out", "d_tries"] + _SAMPLER + ["d_keys", "components", "domain", "index_base", "stream"],
}
CONSTANTS = {"LSR_RING_OPNORM_MAX_DEGREE": "RING_OPNORM_MAX_DEGREE", "LSR_RING_CHALLENGE_ATTEMPT_WORDS": "RING_CHALLENGE_ATTEMPT_WORDS",
             "LSR_RING_CHALLENGE_MAX_TRIES": "RING_CHALLENGE_MAX_TRIES"}
MEMBERS = ("ring_opnorm_prepare", "ring_opnorm", "ring_opnorm_device", "ring_challenge", "ring_challenge_device")
Q14, N = 12289, 64
POWERS = [1 << k for k in range(1, 13)]


class Fake:
    """The library, a buffer address, and a context of zeros but for its modulus and degree."""

    def __init__(self, pkg, q=Q14, n=N):
        self.pkg, self.lib = pkg, pkg._abi.load_library()
        self.buf = (ctypes.c_uint64 * 16)()
        self.ctx_buf = (ctypes.c_uint64 * 128)()
        self.p, self.ctx = ctypes.addressof(self.buf), ctypes.addressof(self.ctx_buf)
        self.set(q, n)

    def set(self, q, n):
        self.ctx_buf[0], self.ctx_buf[1] = q, n              # uint64 modulus; uint32 degree (the log n behind it stays 0)

    def challenge(self, device, ctx, out, tries, keys, count=1, k1=31, k2=10, bound=15, max_tries=64, components=1, index_base=0):
        if device:
            return self.lib.lsr_ntt_ring_challenge_batch_device(ctx, out, tries, count, k1, k2, bound, max_tries, keys, components, 16, index_base, None)
        return self.lib.lsr_ntt_ring_challenge_batch(ctx, out, tries, count, k1, k2, bound, max_tries, keys, components, 16, index_base)

    def refused(self, device, word, *others, **kw):
        """the call is refused with `word` in the message and none of `others`"""
        p = self.p
        assert self.challenge(device, self.ctx, p, p, p, **kw) == -1, kw
        msg = self.pkg._abi.last_error()
        assert msg.startswith(CHALLENGE + ("_device:" if device else ":")) and word in msg, (kw, msg)
        for other in others:
            assert other not in msg, (kw, msg)


@pytest.fixture()
def fake(pkg):
    f = Fake(pkg)
    yield f
    del f


def test_batch_h_declares_the_functions_with_their_argument_names_and_the_contract():
    raw = open(BATCH_H).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, want in ARGUMENTS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
        assert m, name
        assert [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")] == want, name
    for word in ("operator norm", "round(2^30 cos(pi j / n))", "C[(i e) mod 2n]", "C[(i e - n/2) mod 2n]", "N(c) <= T^2 2^60", "{2k + 1 : 0 <= k < n/2}",
                 "{2k : 0 <= k <= n/2}", "t LSR_RING_CHALLENGE_ATTEMPT_WORDS", "c[i] = c[j]", "U = 63", "below 2^28", "2^-72", "re-keys", "SYNCHRONOUSLY"):
        assert word in raw, word                               # the definitions are the contract and live in the header


def test_library_exports_signatures_members_and_constants(pkg):
    lib = pkg._abi.load_library()
    for name, want in ARGUMENTS.items():
        assert hasattr(lib, name), name
        assert len(pkg._abi.SIGNATURES[name][1]) == len(want), name
    for cls in (pkg.NttContext, pkg.CyclicNtt):
        assert issubclass(cls, pkg._RingChallenge)
        for member in MEMBERS:
            assert callable(getattr(cls, member)), member
    text = open(BATCH_H).read()
    for macro, mirror in CONSTANTS.items():
        assert int(re.search(r"#define\s+" + macro + r"\s+(\d+)", text).group(1)) == getattr(pkg, mirror), macro
        assert mirror in pkg.__all__
    assert (pkg.RING_OPNORM_MAX_DEGREE, pkg.RING_CHALLENGE_ATTEMPT_WORDS, pkg.RING_CHALLENGE_MAX_TRIES) == (model.MAX_DEGREE, model.ATTEMPT_WORDS,
                                                                                                          model.MAX_TRIES)
    assert "ring_opnorm_table" in pkg.__all__
    # an attempt's words fit its share of the stream, and all attempts stay below the block counter's 2^28 words
    assert pkg.RING_SAMPLE_MAX_WORDS * pkg.RING_OPNORM_MAX_DEGREE <= pkg.RING_CHALLENGE_ATTEMPT_WORDS
    assert pkg.RING_CHALLENGE_MAX_TRIES * pkg.RING_CHALLENGE_ATTEMPT_WORDS <= 1 << 28


# ---- the table -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", POWERS)
def test_table_is_the_models_and_the_exact_one(pkg, n):
    import mpmath
    got = pkg.ring_opnorm_table(n)
    assert got.dtype == np.int32 and got.shape == (2 * n,)
    assert got.tolist() == model.table(n).tolist()
    mpmath.mp.dps = 50
    exact = [int(mpmath.floor(mpmath.ldexp(mpmath.cos(mpmath.pi * j / n), 30) + mpmath.mpf(1) / 2)) for j in range(2 * n)]
    assert got.tolist() == exact
    assert got[0] == 1 << 30 and got[n] == -(1 << 30) and got[n // 2] == 0 and got[3 * n // 2] == 0


def test_table_refuses_what_is_no_power_of_two_in_range(pkg):
    lib = pkg._abi.load_library()
    out = (ctypes.c_int32 * 16)()
    for n in (0, 1, 3, 6, 4095, 8192, 1 << 31):
        assert lib.lsr_ring_opnorm_table(n, out) == -1, n
        msg = pkg._abi.last_error()
        assert msg.startswith(TABLE + ":") and "power of two" in msg and "4096" in msg, msg
        assert list(out) == [0] * 16
    assert lib.lsr_ring_opnorm_table(4, None) == -1 and "NULL" in pkg._abi.last_error()
    for n in (1, 3, 8192):
        with pytest.raises(pkg.CoreError, match="power of two"):
            pkg.ring_opnorm_table(n)


# ---- the norm and prepare: NULL, the degree, then the empty call --------------------------------------------------------------------------------
def _norm(f, device, ctx, x, count, out):
    if device:
        return f.lib.lsr_ntt_ring_opnorm_batch_device(ctx, x, count, out, None)
    return f.lib.lsr_ntt_ring_opnorm_batch(ctx, x, count, out)


@pytest.mark.parametrize("device", [False, True])
def test_norm_refusals_in_order(pkg, fake, device):
    f, p = fake, fake.p
    name = NORM + ("_device:" if device else ":")
    f.set(Q14, 8192)                                         # the degree would be refused too: NULL is reported first
    for ctx, x, out in [(None, p, p), (f.ctx, None, p), (f.ctx, p, None)]:
        for count in (0, 1, 2**64 - 1):
            assert _norm(f, device, ctx, x, count, out) == -1
            msg = pkg._abi.last_error()
            assert msg.startswith(name) and "NULL" in msg, msg
    for n in (8192, 1 << 17, 1 << 22):                       # before the empty call and the overflowing size
        f.set(Q14, n)
        for count in (0, 1, 2**64 - 1):
            assert _norm(f, device, f.ctx, p, count, p) == -1
            msg = pkg._abi.last_error()
            assert msg.startswith(name) and "LSR_RING_OPNORM_MAX_DEGREE" in msg and "4096" in msg, msg
    for n in (2, 64, 4096):
        f.set(Q14, n)
        assert _norm(f, device, f.ctx, p, 0, p) == 0         # a no-op, out on top of x or not
        assert _norm(f, device, f.ctx, p, 2**64 - 1, p) == -1 and "overflow" in pkg._abi.last_error()
        assert _norm(f, device, f.ctx, p, 1, p) == -1 and "overlaps" in pkg._abi.last_error()


def test_prepare_refuses_null_and_the_degree(pkg, fake):
    lib = fake.lib
    assert lib.lsr_ntt_ring_opnorm_prepare(None) == -1 and "NULL" in pkg._abi.last_error()
    fake.set(Q14, 8192)
    assert lib.lsr_ntt_ring_opnorm_prepare(fake.ctx) == -1
    msg = pkg._abi.last_error()
    assert msg.startswith(PREPARE + ":") and "LSR_RING_OPNORM_MAX_DEGREE" in msg, msg


# ---- the sampler: refusals (1) - (7), then the empty call, then the index ------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True])
def test_challenge_null_is_refused_first(pkg, fake, device):
    f, p = fake, fake.p
    f.set(3, 8192)                                           # every later rule would refuse too
    for ctx, out, tries, keys in [(None, p, p, p), (f.ctx, None, p, p), (f.ctx, p, None, p), (f.ctx, p, p, None)]:
        for kw in [{}, dict(count=0), dict(components=0), dict(k1=0, k2=0), dict(max_tries=0), dict(bound=1 << 32), dict(k1=9000, max_tries=2000, components=0)]:
            assert f.challenge(device, ctx, out, tries, keys, **kw) == -1
            msg = pkg._abi.last_error()
            assert msg.startswith(CHALLENGE + ("_device:" if device else ":")) and "NULL" in msg, msg


@pytest.mark.parametrize("device", [False, True])
def test_challenge_refusals_in_the_documented_order(pkg, fake, device):
    f = fake
    # (2) components == 0, before everything that follows (each of which would refuse too) and before the empty call
    f.set(3, 8192)
    for kw in [{}, dict(count=0), dict(k1=0, k2=0), dict(k1=8193, k2=0), dict(max_tries=0), dict(bound=1 << 32)]:
        f.refused(device, "components", "kappa", "max_tries", "opnorm_bound", "DEGREE", components=0, **kw)
    # (3) kappa1 + kappa2 == 0 or above n, before (4) - (7)
    for q, n, k1, k2 in [(3, 8192, 0, 0), (3, 8192, 8000, 193), (Q14, 64, 64, 1), (Q14, 64, 0, 65), (Q14, 2, 2, 1), (3, 8192, 2**32 - 1, 2**32 - 1)]:
        f.set(q, n)
        for kw in [{}, dict(count=0), dict(max_tries=0), dict(max_tries=1025), dict(bound=1 << 32)]:
            f.refused(device, "kappa1 + kappa2", "modulus", "max_tries", "opnorm_bound", "DEGREE", k1=k1, k2=k2, **kw)
    # (4) kappa2 > 0 with q < 5, before (5) - (7)
    for q in (2, 3, 4):
        f.set(q, 8192)
        for kw in [{}, dict(count=0), dict(max_tries=0), dict(bound=1 << 32), dict(k1=0, k2=1)]:
            f.refused(device, "modulus", "max_tries", "opnorm_bound", "DEGREE", **kw)
    f.set(3, 64)
    assert f.challenge(device, f.ctx, f.p, f.p, f.p, count=0, k1=5, k2=0) == 0      # q = 3 serves +-1 alone
    # (5) max_tries == 0 or above the cap, before (6), (7)
    f.set(Q14, 8192)
    for max_tries in (0, 1025, 2**32 - 1):
        for kw in [{}, dict(count=0), dict(bound=1 << 32), dict(bound=2**64 - 1)]:
            f.refused(device, "max_tries", "opnorm_bound", "DEGREE", max_tries=max_tries, **kw)
    # (6) opnorm_bound >= 2^32, before (7)
    for bound in (1 << 32, 1 << 63, 2**64 - 1):
        for kw in [{}, dict(count=0), dict(max_tries=1024)]:
            f.refused(device, "opnorm_bound", "DEGREE", bound=bound, **kw)
    # (7) the degree, before the empty call
    for n in (8192, 1 << 17):
        f.set(Q14, n)
        for kw in [{}, dict(count=0), dict(bound=0), dict(bound=2**32 - 1, max_tries=1024, k1=n - 10)]:
            f.refused(device, "LSR_RING_OPNORM_MAX_DEGREE", **kw)


@pytest.mark.parametrize("device", [False, True])
def test_challenge_empty_call_is_a_no_op_before_the_index_check(pkg, fake, device):
    f, p = fake, fake.p
    for q, n, k1, k2, bound, max_tries in [(Q14, 64, 31, 10, 15, 256), (5, 2, 1, 1, 2**32 - 1, 1024), (Q14, 4096, 0, 4096, 0, 1), (3, 8, 8, 0, 1, 1)]:
        f.set(q, n)
        for index_base, components in [(0, 1), (2**64 - 1, 5), (2**64 - 16, 16)]:
            assert f.challenge(device, f.ctx, p, p, p, count=0, k1=k1, k2=k2, bound=bound, max_tries=max_tries, components=components,
                               index_base=index_base) == 0
    f.set(Q14, 64)
    for index_base, components in [(2**64 - 1, 1), (2**64 - 16, 16), (1, 2**64 - 1)]:
        f.refused(device, "index_base + components overflows", count=1, components=components, index_base=index_base)


def test_python_wrapper_checks_the_key_count_before_the_library_reads_it(pkg):
    class Ctx(pkg._RingChallenge):
        n, _h, _lib = 16, None, None
    with pytest.raises(ValueError, match="ceil"):
        Ctx().ring_challenge(5, 3, 1, 4, np.zeros((2, 4), dtype=np.uint64), components=2)
    with pytest.raises(ValueError, match="32 bytes"):
        Ctx().ring_challenge(1, 3, 1, 4, b"short")
    with pytest.raises(ValueError, match=r"\[n\]"):
        Ctx().ring_opnorm(np.zeros(15, dtype=np.uint64))
