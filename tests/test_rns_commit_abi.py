"""CPU suite: the two-prime RNS commitment context's ABI surface, its moduli rule and the pure-Python pin of its definition
(tests/rns_model.py, the model the GPU tests compare the library with).  No device work."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import rns_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _batch_h():
    text = open(os.path.join(ROOT, "include", "lambda_snark", "batch.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"\s+", " ", text)


def test_new_symbols_are_declared_exported_and_bound(pkg, lib):
    h = _batch_h()
    assert "LweContext* lsr_lwe_context_create_rns(const PublicParams* params, uint64_t key_seed, int device) LSR_NOEXCEPT;" in h
    assert "int lsr_lwe_rns_moduli(const LweContext* ctx, uint64_t out[2]) LSR_NOEXCEPT;" in h
    sig = pkg._abi.SIGNATURES
    assert sig["lsr_lwe_context_create_rns"] == (ctypes.c_void_p, [ctypes.POINTER(pkg.PublicParams), ctypes.c_uint64, ctypes.c_int])
    assert sig["lsr_lwe_rns_moduli"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p])
    for name in ("lsr_lwe_context_create_rns", "lsr_lwe_rns_moduli"):
        assert hasattr(lib, name)
    assert callable(pkg.LweContext.create_rns) and callable(pkg.LweContext.rns_moduli)


def test_constructor_refuses_without_a_device_and_bad_parameters(pkg, lib):
    assert not lib.lsr_lwe_context_create_rns(None, 1, -1)
    assert lib.lsr_last_error()
    out = (ctypes.c_uint64 * 2)()
    assert lib.lsr_lwe_rns_moduli(None, out) == -1
    # (n, k, sigma) a default context refuses: refused before any device work, each with the text of its own reason
    for n, k, sigma, why in [(4095, 2, 3.19, b"ring_degree"), (0, 2, 3.19, b"ring_degree"), (262144, 2, 3.19, b"ring_degree"), (4096, 17, 3.19, b"module_rank"),
                             (4096, 2, 0.0, b"sigma"), (4096, 2, float("nan"), b"sigma"), (4096, 2, 300.0, b"sigma"), (4096, 2, 200.0, b"noise budget")]:
        ffi = pkg.PublicParams(1, 128, 0, n, k, sigma)
        assert not lib.lsr_lwe_context_create_seeded(ctypes.byref(ffi), 3, -1), (n, k, sigma)
        assert not lib.lsr_lwe_context_create_rns(ctypes.byref(ffi), 3, -1), (n, k, sigma)
        assert why in lib.lsr_last_error(), (n, k, sigma, lib.lsr_last_error())
        assert not lib.lsr_lwe_context_create_rns(None, 3, -1) and b"NULL params" in lib.lsr_last_error()      # another text in between
    if lib.lsr_device_count() > 0:
        return
    ffi = pkg.PublicParams(1, 128, 12345, 4096, 2, 3.19)
    assert not lib.lsr_lwe_context_create_rns(ctypes.byref(ffi), 3, -1)
    assert b"no HIP device" in lib.lsr_last_error()
    with pytest.raises(pkg.CoreError):
        pkg.LweContext.create_rns(pkg.Params(n=4096, k=2), key_seed=3)


def test_moduli_rule(pkg, lib):
    for n in (256, 1024, 4096, 8192, 65536, 131072):
        q1, q2 = rns_model.rns_moduli(n)
        for q in (q1, q2):
            assert 2**43 < q < 2**44 and (q - 1) % (2 * n) == 0 and rns_model.is_prime(q)
        assert q1 != q2
        assert q1 == lib.lsr_select_commit_modulus(0, n)
        assert q2 == rns_model.largest_prime_1mod(2 * n, 44, skip=(q1,))
        # the library's host-only query, word for word
        assert pkg.rns_commit_moduli(n) == (q1, q2)
        # a requested prime of this form is honoured by the single-prime selection (the sibling contexts of the GPU tests rely on it)
        assert lib.lsr_select_commit_modulus(q2, n) == q2
    out = (ctypes.c_uint64 * 2)()
    for n in (0, 3, 4097, 262144):
        assert lib.lsr_rns_commit_moduli(n, out) == -1


def test_python_pin_of_the_definition():
    """round(Q m/t) mod q_i, the CRT lift and the rounded decode: m and noise up to +-(Q/2t - 1) decode to m, just beyond does not."""
    rnd = random.Random(13)
    for n in (1024, 4096, 65536):
        q1, q2 = rns_model.rns_moduli(n)
        t = rns_model.plain_modulus(n)
        big = q1 * q2
        margin = big // (2 * t)
        for m in [0, 1, t - 1] + [rnd.randrange(t) for _ in range(8)]:
            scaled = rns_model.round_div(big * m, t)
            assert abs(scaled * t - big * m) * 2 <= t
            assert rns_model.message_term(m, t, q1, q2, q1) == scaled % q1 and rns_model.message_term(m + 5 * t, t, q1, q2, q2) == scaled % q2
            for noise in (0, 1, -1, margin - 1, -(margin - 1)):
                x = (scaled + noise) % big
                assert rns_model.crt_lift(x % q1, x % q2, q1, q2) == x
                assert rns_model.decode(x % q1, x % q2, t, q1, q2) == m, (n, m, noise)
            # the first noise values that must fail, exactly: decode = floor((t (scaled + e) + floor(Q/2)) / Q) mod t leaves m when
            # t (scaled + e) + floor(Q/2) reaches (m + 1) Q, or falls below m Q
            up = -((-((m + 1) * big - big // 2 - t * scaled)) // t)                 # ceil
            down = (t * scaled + big // 2 - m * big) // t + 1
            # |t scaled - Q m| <= t/2 (the rounding of the scaled message): both lie within Q/2t -+ 1/2, rounded up
            assert margin - 1 < up <= margin + 2 and margin - 1 < down <= margin + 2
            for noise, opens in ((up - 1, True), (up, False), (-(down - 1), True), (-down, False)):
                x = (scaled + noise) % big
                assert (rns_model.decode(x % q1, x % q2, t, q1, q2) == m) == opens, (n, m, noise)
    assert rns_model.header(4096, 2, 1032193, 5, 7) == [8 * (6 + 2 * 3 * 4096 - 1), int.from_bytes(b"LSRR0001", "little"), 4096 | (2 << 32), 5, 7, 1032193]
