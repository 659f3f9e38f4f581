"""CPU suite: the ABI surface of row decoding (lsr_lwe_decode_rows_device, lsr_lwe_decode_batch_flat, lsr_lwe_decode,
lsr_lwe_noise_capacity_bits) and the pure-Python pin of its definitions (decode_model.py, the model the GPU tests compare the
library with).  No device work."""
import ctypes
import os
import random
import re

import numpy as np

import decode_model
import rns_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLARATIONS = [
    "int lsr_lwe_decode_rows_device(const LweContext* ctx, const uint64_t* d_rows, size_t count, size_t slots, uint64_t* d_messages, int* d_status, "
    "uint32_t* d_noise_bits, void* stream) LSR_NOEXCEPT;",
    "int lsr_lwe_decode_batch_flat(const LweContext* ctx, const uint64_t* words, size_t count, size_t slots, uint64_t* messages, int* status, "
    "uint32_t* noise_bits) LSR_NOEXCEPT;",
    "int lsr_lwe_decode(const LweContext* ctx, const LweCommitment* cm, uint64_t* message, size_t slots, uint32_t* noise_bits) LSR_NOEXCEPT;",
    "uint32_t lsr_lwe_noise_capacity_bits(const LweContext* ctx) LSR_NOEXCEPT;",
]


def _batch_h():
    text = open(os.path.join(ROOT, "include", "lambda_snark", "batch.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"\s+", " ", text)


def test_symbols_are_declared_exported_and_bound(pkg, lib):
    h = _batch_h()
    for line in DECLARATIONS:
        assert line in h, line
    vp, size, cint = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    sig = pkg._abi.SIGNATURES
    assert sig["lsr_lwe_decode_rows_device"] == (cint, [vp, vp, size, size, vp, vp, vp, vp])
    assert sig["lsr_lwe_decode_batch_flat"] == (cint, [vp, vp, size, size, vp, vp, vp])
    assert sig["lsr_lwe_decode"] == (cint, [vp, ctypes.POINTER(pkg._abi.LweCommitment), vp, size, vp])
    assert sig["lsr_lwe_noise_capacity_bits"] == (ctypes.c_uint32, [vp])
    for name in ("lsr_lwe_decode_rows_device", "lsr_lwe_decode_batch_flat", "lsr_lwe_decode", "lsr_lwe_noise_capacity_bits"):
        assert hasattr(lib, name)
    assert callable(pkg.LweContext.decode_rows_device) and callable(pkg.LweContext.decode_rows) and callable(pkg.Commitment.decode)
    assert isinstance(pkg.LweContext.noise_capacity_bits, property)


def test_definitions_are_stated_in_the_header_and_the_design():
    header = open(os.path.join(ROOT, "include", "lambda_snark", "batch.h")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for text in (header, design):
        for needle in ("rho_i", "noise_bits", "rem_i", "bitlen"):
            assert needle in text, needle
    assert "6b" in design and "Decoding rows and the measured noise" in design


def test_a_null_context_is_refused_with_a_message_and_no_device(lib):
    """Without a device no context can exist, so the NULL context is the one argument error a host without a GPU can reach; the refusals
    that need a live context (NULL buffers, slots 0 and > ring_degree) are in the GPU suite."""
    buf = np.zeros(8, dtype=np.uint64)
    status = np.zeros(1, dtype=np.int32)
    bits = np.zeros(1, dtype=np.uint32)
    calls = {
        b"lsr_lwe_decode_rows_device": lambda: lib.lsr_lwe_decode_rows_device(None, buf.ctypes.data, 1, 1, buf.ctypes.data, status.ctypes.data, bits.ctypes.data, None),
        b"lsr_lwe_decode_batch_flat": lambda: lib.lsr_lwe_decode_batch_flat(None, buf.ctypes.data, 1, 1, buf.ctypes.data, status.ctypes.data, bits.ctypes.data),
        b"lsr_lwe_decode": lambda: lib.lsr_lwe_decode(None, None, buf.ctypes.data, 1, bits.ctypes.data),
    }
    for name, call in calls.items():
        assert not lib.lsr_lwe_context_create_rns(None, 3, -1) and b"NULL params" in lib.lsr_last_error()      # another text in between
        assert call() == -1
        assert name in lib.lsr_last_error() and b"NULL context" in lib.lsr_last_error(), lib.lsr_last_error()
    # count == 0 does not rescue a NULL context
    assert lib.lsr_lwe_decode_rows_device(None, buf.ctypes.data, 0, 1, buf.ctypes.data, status.ctypes.data, None, None) == -1
    assert lib.lsr_lwe_noise_capacity_bits(None) == 0


def test_python_pin_of_the_definitions():
    """slot and rho of decode_model against first principles: slot = round(t x / q) mod t, rho = |t x - s q| <= floor(q/2), and a message
    with noise e scaled in decodes to the message with rho = |t e + (t scaled - q m)| while that stays below q/2."""
    rnd = random.Random(7)
    for n in (1024, 4096):
        t = rns_model.plain_modulus(n)
        q1, q2 = rns_model.rns_moduli(n)
        for q in (q1, (1 << 60) - 93, q1 * q2):                      # 44-bit, a 60-bit modulus, the RNS product
            half = q // 2
            assert decode_model.capacity_bits(q) == half.bit_length()
            for x in [0, 1, q - 1, half, half - 1, half + 1] + [rnd.randrange(q) for _ in range(64)]:
                slot, rho = decode_model.slot_and_rho(x, t, q)
                s = (t * x + half) // q
                assert 0 <= s <= t and slot == s % t and rho == abs(t * x - s * q) <= half
                # the nearest multiple of q to t x is s q (ties cannot occur: rho <= floor(q/2) and q is odd)
                assert all(abs(t * x - c * q) >= rho for c in (s - 1, s + 1))
            for m in (0, 1, t - 1, rnd.randrange(t)):
                scaled = rns_model.round_div(q * m, t)
                for e in (0, 1, -1, 1000, -(half // t - 2)):
                    slot, rho = decode_model.slot_and_rho((scaled + e) % q, t, q)
                    assert slot == m and rho == abs(t * e + t * scaled - q * m)
    assert decode_model.noise_bits([0, 0], 5, 11) == 0
    assert decode_model.noise_bits([0, 2], 5, 11) == 1              # 5 * 2 = 10 = 1 * 11 - 1
