"""CPU suite: the ABI surface of the batched linear combination of commitment rows (lsr_lwe_combine_rows_device,
lsr_lwe_combine_batch_flat), the refusals a host without a device can reach, and the pure-Python pin of the model the GPU tests compare
the library with (combine_model.py).  No device work."""
import ctypes
import os
import random
import re

import numpy as np

import combine_model
import rns_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLARATIONS = [
    "int lsr_lwe_combine_rows_device(const LweContext* ctx, const uint64_t* d_rows, size_t terms, size_t term_stride, const uint64_t* d_coeffs, "
    "size_t outputs, uint64_t* d_out_rows, int* d_status, void* stream) LSR_NOEXCEPT;",
    "int lsr_lwe_combine_batch_flat(const LweContext* ctx, const uint64_t* rows, size_t terms, size_t term_stride, const uint64_t* coeffs, "
    "size_t outputs, uint64_t* out_rows, int* status) LSR_NOEXCEPT;",
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
    assert sig["lsr_lwe_combine_rows_device"] == (cint, [vp, vp, size, size, vp, size, vp, vp, vp])
    assert sig["lsr_lwe_combine_batch_flat"] == (cint, [vp, vp, size, size, vp, size, vp, vp])
    for name in ("lsr_lwe_combine_rows_device", "lsr_lwe_combine_batch_flat"):
        fn = getattr(lib, name)
        assert fn.restype is cint and list(fn.argtypes) == sig[name][1]
    assert callable(pkg.LweContext.combine_rows_device) and callable(pkg.LweContext.combine_rows)


def test_tile_constants_agree_between_header_kernel_and_binding(pkg):
    """the recentring interval and the output tile the GPU tests sweep around: one value in batch.h, the kernel header and _abi.py"""
    h = _batch_h()
    kernel = open(os.path.join(ROOT, "lambda-snark-r_amd", "csrc", "lsr_commit_combine.hpp")).read()
    for macro, constant, value in (("LSR_COMBINE_TERMS", "kCombineTerms", pkg._abi.COMBINE_TERMS), ("LSR_COMBINE_OUTPUTS", "kCombineOutputs", pkg._abi.COMBINE_OUTPUTS)):
        assert f"#define {macro} {value} " in h
        assert re.search(rf"constexpr uint32_t {constant} = {value};", kernel)
    # the accumulation bound of DESIGN.md section 6c: a carried canonical residue plus R products of at most 0.875 q stay within 32 q
    assert 1 + pkg._abi.COMBINE_TERMS * 0.875 <= 32


def test_contract_is_stated_in_the_header_and_the_design():
    header = open(os.path.join(ROOT, "include", "lambda_snark", "batch.h")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for text in (header, design):
        for needle in ("lsr_lwe_combine_rows_device", "lsr_lwe_combine_batch_flat", "term_stride", "centred"):
            assert needle in text, needle
    assert "### 6c." in design and "0.875" in design[design.index("### 6c."):]


def test_refusals_without_a_device(lib):
    """Without a device no context can exist, so the NULL context is the one argument error a host without a GPU can reach; the refusals
    that need a live context (NULL buffers, terms = 0, an overflowing stride) are in the GPU suite."""
    buf = np.zeros(8, dtype=np.uint64)
    status = np.full(1, 7, dtype=np.int32)
    calls = {
        b"lsr_lwe_combine_rows_device": lambda outputs: lib.lsr_lwe_combine_rows_device(None, buf.ctypes.data, 1, 0, buf.ctypes.data, outputs, buf.ctypes.data,
                                                                                        status.ctypes.data, None),
        b"lsr_lwe_combine_batch_flat": lambda outputs: lib.lsr_lwe_combine_batch_flat(None, buf.ctypes.data, 1, 0, buf.ctypes.data, outputs, buf.ctypes.data,
                                                                                      status.ctypes.data),
    }
    for name, call in calls.items():
        for outputs in (1, 0):                    # outputs == 0 does not rescue a NULL context
            assert not lib.lsr_lwe_context_create_rns(None, 3, -1) and b"NULL params" in lib.lsr_last_error()      # another text in between
            assert call(outputs) == -1
            assert name in lib.lsr_last_error() and b"NULL context" in lib.lsr_last_error(), lib.lsr_last_error()
    assert status[0] == 7 and not buf.any()       # nothing was written


def test_python_pin_of_the_model():
    """combine_model against first principles: the centred representative, the weight, and a combination mod q that a signed big-integer
    sum reproduces; the two budget comparisons are monotone, so `largest accepted weight` is well defined."""
    rnd = random.Random(5)
    t = rns_model.plain_modulus(4096)
    assert [combine_model.centred(c, t) for c in (0, 1, t // 2, t // 2 + 1, t - 1, t, t + 1, 2**64 - 1)] == \
        [0, 1, t // 2, -(t // 2), -1, 0, 1, combine_model.centred((2**64 - 1) % t, t)]
    q1, q2 = rns_model.rns_moduli(4096)
    for q in (q1, q2, (1 << 60) - 93):
        terms = [[rnd.randrange(q) for _ in range(5)] for _ in range(7)]
        coeffs = [rnd.randrange(2**64) for _ in range(7)]
        got = combine_model.combine(terms, coeffs, t, q)
        for x in range(5):
            assert got[x] == sum(((c % t) - (t if (c % t) > t // 2 else 0)) * row[x] for c, row in zip(coeffs, terms)) % q
        assert combine_model.weight(coeffs, t) == sum(abs(combine_model.centred(c, t)) for c in coeffs)
