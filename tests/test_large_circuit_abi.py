"""CPU suite for circuits of up to 2^22 constraints on the NTT path (include/lambda_snark/prover.h: lsr_prover_max_log2_size,
lsr_cyclic_ntt_context_create_large, lsr_quotient_plan_create_large): the symbols are declared, exported and mirrored, the argument
checks of the two constructors answer before any device work, and the host verifier takes a record of a 2^20-constraint circuit.

It also carries what the GPU suite (test_large_circuit_gpu.py) measures against: a vectorised circuit builder, array forms of the
oracle's sparse product, and an exact O(m log m) quotient built only from the oracle's cyclic transforms and Python integers — the
oracle's own quotient is schoolbook O(m^2) — pinned here against that oracle quotient at m = 64 and 4096."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROVER_H = os.path.join(ROOT, "include", "lambda_snark", "prover.h")
Q = 18446744069414584321
M64 = (1 << 64) - 1
ENTRY = np.dtype([("row", "<u4"), ("col", "<u4"), ("value", "<u8")])     # r1cs.h SparseEntry

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prover_replay  # noqa: E402


# ---- shared with the GPU suite ------------------------------------------------------------------------------------------------------
def sparse_mul_vec(oracle, entries, n_rows, v):
    """SparseMatrix::mul_vec through the oracle's array entry point (the list-of-tuples wrapper is too slow at 4 M entries)"""
    rows, cols, vals = (np.ascontiguousarray(entries[k]) for k in ("row", "col", "value"))
    vec = np.ascontiguousarray(v, dtype=np.uint64)
    out = np.zeros(n_rows, dtype=np.uint64)
    oracle.L.oracle_sparse_mul_vec(rows.ctypes.data, cols.ctypes.data, vals.ctypes.data, len(entries), vec.ctypes.data, Q, out.ctypes.data, n_rows)
    return out


def pointwise_mul(oracle, x, y):
    """x_i y_i mod q for arrays: the oracle's sparse product of diag(x) with y"""
    idx = np.arange(len(x), dtype=np.uint32)
    d = np.zeros(len(x), dtype=ENTRY)
    d["row"], d["col"], d["value"] = idx, idx, x
    return sparse_mul_vec(oracle, d, len(x), y)


def build_circuit(rng, m, free_vars=8, fan_in=2):
    """m constraints (A_i.z)(B_i.z) = z[free_vars + i] over free_vars + m variables, A_i and B_i on the free variables only, so a
    witness is one sparse product per matrix and one pointwise product.  Values are any 64-bit words (`val % modulus`).  numpy only."""
    n = free_vars + m
    mats = []
    for _ in range(2):
        e = np.zeros(m * fan_in, dtype=ENTRY)
        e["row"] = np.repeat(np.arange(m, dtype=np.uint32), fan_in)
        e["col"] = rng.integers(0, free_vars, size=m * fan_in, dtype=np.uint32)      # a repeated (row, col) adds up
        e["value"] = rng.integers(0, 2**64, size=m * fan_in, dtype=np.uint64)
        mats.append(e)
    c = np.zeros(m, dtype=ENTRY)
    c["row"] = np.arange(m, dtype=np.uint32)
    c["col"] = np.arange(free_vars, n, dtype=np.uint32)
    c["value"] = 1
    return n, (mats[0], mats[1], c)


def make_witness(oracle, free, m, mats):
    z = np.zeros(len(free) + m, dtype=np.uint64)
    z[:len(free)] = np.asarray(free, dtype=np.uint64) % np.uint64(Q)
    z[len(free):] = pointwise_mul(oracle, sparse_mul_vec(oracle, mats[0], m, z), sparse_mul_vec(oracle, mats[1], m, z))
    return z


def fast_quotient(oracle, ea, eb, ec):
    """compute_quotient_poly on the NTT path (r1cs.rs:489-503) in O(m log m): interpolate, multiply through transforms of size 2m, subtract C,
    divide by X^m - 1.  -> (coefficients [m], trimmed length or 0 on a remainder, (A, B, C) interpolants)"""
    m = len(ea)
    w_m, w_2m = oracle.prover_omega(m), oracle.prover_omega(2 * m)
    pa, pb, pc = (oracle.cyclic_inverse(v, Q, w_m) for v in (ea, eb, ec))
    pad = np.zeros(m, dtype=np.uint64)
    fa = oracle.cyclic_forward(np.concatenate([pa, pad]), Q, w_2m).astype(object)
    fb = oracle.cyclic_forward(np.concatenate([pb, pad]), Q, w_2m).astype(object)
    prod = (fa * fb) % Q                                                     # Python integers
    num = oracle.cyclic_inverse(np.array(prod, dtype=np.uint64), Q, w_2m).astype(object)
    num[:m] = (num[:m] - pc.astype(object)) % Q
    # N = Q (X^m - 1)  =>  N_{i+m} = Q_i - Q_{i+m}: Q_i = N_{i+m} + Q_{i+m} from the top down, Q_j = 0 for j >= m (deg N < 2m)
    quot = np.zeros(2 * m, dtype=object)
    quot[:m] = (num[m:] + quot[m:]) % Q
    clean = not np.any((num[:m] + quot[:m]) % Q)                             # remainder: N_i + Q_i = 0 for i < m
    coeffs = np.array(quot[:m], dtype=np.uint64)
    if not clean:
        return coeffs, 0, (pa, pb, pc)
    nz = np.flatnonzero(coeffs)
    return coeffs, (int(nz[-1]) + 1 if len(nz) else 1), (pa, pb, pc)


# ---- the declarations ---------------------------------------------------------------------------------------------------------------
def test_prover_h_declares_the_large_constructors():
    text = re.sub(r"/\*.*?\*/", "", open(PROVER_H).read(), flags=re.S)
    assert re.search(r"\buint32_t\s+lsr_prover_max_log2_size\s*\(\s*void\s*\)", text)
    assert re.search(r"\bNttContext\s*\*\s*lsr_cyclic_ntt_context_create_large\s*\(\s*uint64_t\s+q\s*,\s*uint32_t\s+n\s*,\s*uint64_t\s+omega\s*,\s*int\s+device\s*\)", text)
    assert re.search(r"\bLsrQuotientPlan\s*\*\s*lsr_quotient_plan_create_large\s*\(\s*uint32_t\s+m\s*,\s*int\s+device\s*\)", text)


def test_library_exports_signatures_and_ceiling(pkg):
    lib = pkg._abi.load_library()
    for name, argc in (("lsr_prover_max_log2_size", 0), ("lsr_cyclic_ntt_context_create_large", 4), ("lsr_quotient_plan_create_large", 2)):
        assert hasattr(lib, name), name
        assert len(pkg._abi.SIGNATURES[name][1]) == argc
    assert lib.lsr_prover_max_log2_size() == 22
    assert pkg.prover_max_log2_size() == 22


def _is_prime(q):
    if q < 2:
        return False
    d, s = q - 1, 0
    while d % 2 == 0:
        d //= 2; s += 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if a % q == 0:
            continue
        x = pow(a, d, q)
        if x in (1, q - 1):
            continue
        for _ in range(s - 1):
            x = x * x % q
            if x == q - 1:
                break
        else:
            return False
    return True


def _goldilocks_free_prime(n):
    """a prime q < 2^61, q = 1 mod n, with an element of exact order n (not the prover's field)"""
    q = (1 << 50) + 1
    while not _is_prime(q):
        q -= n
    for g in range(2, 1000):
        w = pow(g, (q - 1) // n, q)
        if pow(w, n // 2, q) == q - 1:
            return q, w
    raise AssertionError("no element of order n")


def _expect_null_or_handle(pkg, lib, handle, free):
    """valid arguments: without a device NULL and the no-device text; with one, a handle"""
    if handle:
        free(handle)
    else:
        assert "no HIP device" in pkg._abi.last_error()


def test_cyclic_large_constructor_checks_its_arguments(pkg):
    lib = pkg._abi.load_library()
    create = lib.lsr_cyclic_ntt_context_create_large
    for n in (0, 3, 1 << 23):
        assert not create(Q, n, 0, -1), n
        assert "lsr_cyclic_ntt_context_create_large" in pkg._abi.last_error() and "4194304" in pkg._abi.last_error()
    for n in (1 << 18, 1 << 22):
        omega = pkg.compute_root_of_unity(n)
        assert not create(Q, n, pow(omega, 2, Q), -1)                        # order n / 2
        assert "omega of order n" in pkg._abi.last_error()
        assert not create(Q, n, 1, -1) and not create(Q, n, Q, -1)
    q, w = _goldilocks_free_prime(1 << 18)
    assert not create(q, 1 << 18, 0, -1)                                     # the default root exists for NTT_MODULUS only
    assert "omega of order n" in pkg._abi.last_error()
    assert not create(q, 1 << 18, w, -1)                                     # a good root of another prime: three passes are Goldilocks only
    assert "NTT_MODULUS" in pkg._abi.last_error()
    q17, w17 = _goldilocks_free_prime(1 << 17)                               # ... but at n <= 2^17 it is the namesake's contract
    _expect_null_or_handle(pkg, lib, create(q17, 1 << 17, w17, -1), lib.ntt_context_free)
    for n in (2, 1 << 12, 1 << 17, 1 << 18, 1 << 20, 1 << 22):
        _expect_null_or_handle(pkg, lib, create(Q, n, 0, -1), lib.ntt_context_free)
        _expect_null_or_handle(pkg, lib, create(Q, n, pkg.compute_root_of_unity(n), -1), lib.ntt_context_free)


def test_quotient_plan_large_constructor_checks_its_arguments(pkg):
    lib = pkg._abi.load_library()
    create = lib.lsr_quotient_plan_create_large
    for m in (0, 3, 1 << 23, (1 << 22) + 1):
        assert not create(m, -1), m
        assert "lsr_quotient_plan_create_large" in pkg._abi.last_error() and "4194304" in pkg._abi.last_error()
    for m in (1, 2, 1 << 17, 1 << 18, 1 << 22):
        _expect_null_or_handle(pkg, lib, create(m, -1), lib.lsr_quotient_plan_free)


def test_python_wrappers_route_large_sizes(pkg):
    assert pkg.MAX_TWO_PASS_SIZE == 1 << 17 and pkg.SPARSE_ENTRY_DTYPE == ENTRY and ENTRY.itemsize == ctypes.sizeof(pkg._abi.SparseEntry)
    with pytest.raises(pkg.CoreError, match="lsr_cyclic_ntt_context_create_large"):
        pkg.CyclicNtt(1 << 23)
    with pytest.raises(pkg.CoreError, match="lsr_quotient_plan_create_large"):
        pkg.QuotientPlan(1 << 23)
    with pytest.raises(pkg.CoreError, match=r"lsr_quotient_plan_create\("):
        pkg.QuotientPlan(3)
    rng = np.random.default_rng(1)
    n, mats = build_circuit(rng, 1 << 23, free_vars=2, fan_in=1)             # array matrices are taken as they are; m is refused
    with pytest.raises(pkg.CoreError, match="4194304"):
        pkg.R1csProver(1 << 23, n, *mats)


# ---- the yardstick of the GPU suite -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [64, 4096])
def test_fast_quotient_equals_the_oracle_quotient(oracle, m):
    rng = np.random.default_rng(m)
    n, mats = build_circuit(rng, m)
    for trial in range(3):
        z = make_witness(oracle, rng.integers(0, 2**64, size=8, dtype=np.uint64), m, mats)
        if trial == 2:
            z[n - 5] = np.uint64((int(z[n - 5]) + 1) % Q)                    # one broken constraint
        ea, eb, ec = (sparse_mul_vec(oracle, mat, m, z) for mat in mats)
        for mat, got in zip(mats, (ea, eb, ec)):                             # the array form == the binding's list form
            assert np.array_equal(got, oracle.sparse_mul_vec([(int(e["row"]), int(e["col"]), int(e["value"])) for e in mat], m, z, Q))
        want, want_len = oracle.quotient(ea, eb, ec)
        got, got_len, (pa, pb, pc) = fast_quotient(oracle, ea, eb, ec)
        assert got_len == want_len and (want_len > 0) == (trial != 2)
        if want_len:
            assert np.array_equal(got, want)
            assert np.array_equal(pa, oracle.cyclic_inverse(ea, Q, oracle.prover_omega(m)))
    zero = np.zeros(m, dtype=np.uint64)                                      # A B - C = 0: Ok([0])
    assert fast_quotient(oracle, zero, zero, zero)[1] == 1 == oracle.quotient(zero, zero, zero)[1]
    one = np.ones(m, dtype=np.uint64)                                        # A = B = C = 1: N = 0 as well
    assert fast_quotient(oracle, one, one, one)[1] == 1 == oracle.quotient(one, one, one)[1]
    assert fast_quotient(oracle, one, one, zero)[1] == 0 == oracle.quotient(one, one, zero)[1]   # N = 1: degree below m, Err


# ---- the verifier's side of the GPU suite's proofs ----------------------------------------------------------------------------------
@pytest.mark.parametrize("zk", [False, True])
def test_host_verifier_takes_a_record_of_a_2_pow_20_circuit(pkg, zk):
    """a record made by hand: any values with Q'(x) Z_H(x) relation holding at the two derived challenges verify (lib.rs:1016-1095)"""
    m, batch, words, n_public = 1 << 20, 3, 37, 2
    rng = np.random.default_rng(20)
    rows = rng.integers(0, 2**63, size=(batch, words), dtype=np.uint64)
    publics = rng.integers(0, 2**64, size=(batch, n_public), dtype=np.uint64)
    proofs = np.zeros((batch, 13), dtype=np.uint64)
    for i in range(batch):
        alpha, _ = prover_replay.challenge_derive([int(v) for v in publics[i]], rows[i], Q)
        beta, _ = prover_replay.challenge_derive([alpha], rows[i], Q)
        r = int(rng.integers(0, Q, dtype=np.uint64)) if zk else 0
        rec = {0: alpha, 1: beta, 12: r}
        for k, x in enumerate((alpha, beta)):
            zh = (pow(x, m, Q) - 1) % Q
            a, b, quot = (int(v) for v in rng.integers(0, Q, size=3, dtype=np.uint64))
            rec[4 + 3 * k], rec[5 + 3 * k], rec[6 + 3 * k] = a, b, (a * b - quot * zh) % Q
            rec[2 + k] = rec[10 + k] = (quot + r * zh) % Q                   # Q'(x) = Q(x) + r Z_H(x)
        proofs[i] = [rec[w] for w in range(13)]
    assert list(pkg.verify_r1cs_batch(m, publics, rows, proofs, zk=zk)) == [1] * batch
    for w in range(13):
        if w == 12 and not zk:
            continue                                                         # verify_r1cs does not read the blinding word
        bad = proofs.copy()
        bad[w % batch, w] ^= np.uint64(1)
        want = [1] * batch
        want[w % batch] = 0
        assert list(pkg.verify_r1cs_batch(m, publics, rows, bad, zk=zk)) == want, w
    assert list(pkg.verify_r1cs_batch(m // 2, publics, rows, proofs, zk=zk)) == [0] * batch   # another circuit size
