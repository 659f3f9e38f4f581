"""Writes reference_sampler.json: output of the reference's own Gaussian sampler (cpp-core/src/utils.cpp `sample_gaussian`,
the one source of the reference's path that compiles on its own), recorded once so that tests/test_reference_sampler.py
needs neither the reference's sources nor a binary built from them.  Run from the repo root after `make -C oracle ref`
(REFERENCE=<checkout of the reference>): `python tests/golden/make_reference_sampler.py`.

Recorded per sigma: the histogram of 400 000 draws (the reference draws from std::random_device, so one draw is as good as
another; the test's statistics are distributional).  Plus the return code of every argument case of the C contract."""
import ctypes
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref", "libref_utils.so")
DRAWS = 400_000
SIGMAS = [3.19, 3.2, 1.0, 8.0]
# (pointer given, length, sigma) of tests/test_reference_sampler.py::test_argument_contract_equals_the_reference
CASES = [(False, 16, 3.2), (True, 0, 3.2), (True, 8, 0.0), (True, 8, -1.0), (True, 8, float("inf")), (True, 8, float("nan")),
         (True, 8, 3.19), (True, 1, 0.5)]


def main():
    lib = ctypes.CDLL(REF)
    lib.sample_gaussian.restype = ctypes.c_int
    lib.sample_gaussian.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double]
    out = {"source": "cpp-core/src/utils.cpp sample_gaussian of the reference, built by `make -C oracle ref`; written by make_reference_sampler.py",
           "draws": DRAWS, "histograms": {}, "argument_contract": []}
    for sigma in SIGMAS:
        buf = np.zeros(DRAWS, dtype=np.uint64)
        assert lib.sample_gaussian(buf.ctypes.data, DRAWS, sigma) == 0
        values, counts = np.unique(buf.view(np.int64), return_counts=True)
        out["histograms"][repr(sigma)] = {"values": [int(v) for v in values], "counts": [int(c) for c in counts]}
    buf = np.zeros(8, dtype=np.uint64)
    for given, length, sigma in CASES:
        rc = lib.sample_gaussian(buf.ctypes.data if given else None, length, sigma)
        out["argument_contract"].append({"pointer": given, "length": length, "sigma": repr(sigma), "rc": int(rc)})
    with open(os.path.join(HERE, "reference_sampler.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("wrote reference_sampler.json")


if __name__ == "__main__":
    main()
