"""CPU suite: the Lagrange-path entry points (include/lambda_snark/prover.h) are declared, exported and mirrored,
their argument checks answer before any device work, tests/lagrange_oracle.py agrees with tests/prover_replay.py and with a
literal restatement of lagrange_basis_ntt, and the host verifier lsr_r1cs_verify_batch_mod — which needs no GPU — accepts honest
proofs, rejects every tampered word and equals lsr_r1cs_verify_batch on the NTT path."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROVER_H = os.path.join(ROOT, "include", "lambda_snark", "prover.h")
SYMBOLS = ["lsr_r1cs_prover_create_mod", "lsr_r1cs_prover_modulus", "lsr_r1cs_prover_uses_ntt", "lsr_r1cs_interpolate_batch",
           "lsr_r1cs_verify_batch_mod", "lsr_r1cs_verify_batch_mod_device"]
GOLD = 18446744069414584321
SEQ_MODULI = [(1 << 44) + 1, (1 << 31) - 1, 17592186044423, 97, GOLD]
M64 = (1 << 64) - 1
CQ, CN, CK, SIGMA, KEY_SEED = 17592186044417, 4096, 2, 3.19, 0x5EED

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lagrange_oracle as lo  # noqa: E402
import prover_replay  # noqa: E402


def test_prover_h_declares_the_lagrange_calls():
    text = re.sub(r"/\*.*?\*/", "", open(PROVER_H).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", text), name


def test_library_exports_and_signatures(pkg):
    lib = pkg._abi.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in pkg._abi.SIGNATURES, name
    assert len(pkg._abi.SIGNATURES["lsr_r1cs_prover_create_mod"][1]) == 5
    assert len(pkg._abi.SIGNATURES["lsr_r1cs_verify_batch_mod"][1]) == 10
    assert len(pkg._abi.SIGNATURES["lsr_r1cs_verify_batch_mod_device"][1]) == 11
    assert hasattr(pkg.R1csProver, "interpolate_batch")


def _mats(pkg, m, n, entries=((0, 0, 1),)):
    keep, mats = [], []
    for _ in range(3):
        arr = (pkg._abi.SparseEntry * len(entries))(*[pkg._abi.SparseEntry(r, c, v) for r, c, v in entries])
        keep.append(arr)
        mats.append(pkg._abi.SparseMatrix(ctypes.cast(arr, ctypes.POINTER(pkg._abi.SparseEntry)), len(entries), m, n))
    return keep, mats


def test_create_mod_argument_checks(pkg):
    lib = pkg._abi.load_library()
    for m, q, why in ((4, 1 << 44, "odd"), (4, 2, "odd"), (4, 1, "odd"), (0, 97, "m <= 8192"), (8193, 97, "m <= 8192")):
        keep, mats = _mats(pkg, max(m, 1) if m else 0, 2, ((0, 0, 1),) if m else ())
        assert not lib.lsr_r1cs_prover_create_mod(*(ctypes.byref(x) for x in mats), q, -1)
        assert why in pkg._abi.last_error(), (m, q, pkg._abi.last_error())
    keep, mats = _mats(pkg, 3, 2, ((0, 5, 1),))
    assert not lib.lsr_r1cs_prover_create_mod(*(ctypes.byref(x) for x in mats), 97, -1)
    assert not lib.lsr_r1cs_prover_create_mod(None, None, None, 97, -1)
    assert lib.lsr_r1cs_prover_modulus(None) == 0 and lib.lsr_r1cs_prover_uses_ntt(None) == 0
    # a valid circuit: NULL exactly when no GPU is visible (the library has no CPU fallback)
    keep, mats = _mats(pkg, 3, 2)
    h = lib.lsr_r1cs_prover_create_mod(*(ctypes.byref(x) for x in mats), 97, -1)
    if lib.lsr_device_count() <= 0:
        assert not h and "no HIP device" in pkg._abi.last_error()
    else:
        assert h and lib.lsr_r1cs_prover_modulus(h) == 97 and lib.lsr_r1cs_prover_uses_ntt(h) == 0
        lib.lsr_r1cs_prover_free(h)


@pytest.mark.parametrize("device", [False, True])
def test_verify_mod_argument_checks(pkg, device):
    lib = pkg._abi.load_library()
    p = ctypes.addressof((ctypes.c_uint64 * 64)())
    r = ctypes.addressof((ctypes.c_int * 4)())
    fn = lib.lsr_r1cs_verify_batch_mod_device if device else lib.lsr_r1cs_verify_batch_mod
    extra = [None] if device else []
    for args in ([3, 97, None, 1, p, 4, p, 1, 0, r], [3, 97, p, 1, None, 4, p, 1, 0, r], [3, 97, p, 1, p, 4, None, 1, 0, r],
                 [3, 97, p, 1, p, 4, p, 1, 0, None]):
        assert fn(*(args + extra)) == -1 and "NULL" in pkg._abi.last_error()
    for q in (1 << 44, 2, 1, 0):
        assert fn(*([3, q, p, 1, p, 4, p, 1, 0, r] + extra)) == -1 and "odd" in pkg._abi.last_error()
    assert fn(*([0, 97, p, 1, p, 4, p, 1, 0, r] + extra)) == -1
    assert fn(*([8193, 97, p, 1, p, 4, p, 1, 0, r] + extra)) == -1 and "8192" in pkg._abi.last_error()
    assert fn(*([3, 97, p, 1, p, 0, p, 1, 0, r] + extra)) == -1
    assert fn(*([3, 97, p, 1, p, 4, p, 0, 0, r] + extra)) == 0          # batch 0


# ---- the oracle against the O(m^3) replay and the literal omega-domain basis ----
@pytest.mark.parametrize("q", SEQ_MODULI)
def test_oracle_matches_the_replay_on_the_sequential_domain(q):
    rng = np.random.default_rng(q % 1000)
    for m in (1, 2, 3, 5, 10, 17, 24):
        if q == (1 << 44) + 1 and m >= 18:
            with pytest.raises(lo.NotAUnit):
                lo.interpolation_rows(m, q)
            continue
        if lo.uses_ntt(m, q):
            continue
        assert lo.domain(m, q) == list(range(m))
        ev = [int(v) % q for v in rng.integers(0, 2**63, size=m)]
        assert lo.interpolate(ev, q) == prover_replay.lagrange_interpolate(ev, q)
        # a numerator divisible by Z_H, and one that is not
        qq = [int(v) % q for v in rng.integers(0, 2**63, size=max(1, m - 1))]
        num = lo.poly_mul(qq, lo.vanishing_seq(m, q), q)[:2 * m - 1] if m > 1 else [0]
        num = num + [0] * (2 * m - 1 - len(num))
        want = prover_replay.poly_div_vanishing(num, m, q)
        assert lo.poly_div_vanishing(num, m, q) == want
        bad = list(num)
        bad[0] = (bad[0] + 1) % q
        with pytest.raises(ValueError):
            prover_replay.poly_div_vanishing(bad, m, q)
        assert lo.poly_div_vanishing(bad, m, q) is None


def test_non_unit_denominators_and_the_omega_rule():
    with pytest.raises(lo.NotAUnit):
        lo.interpolation_rows(100, 97)                    # 97 | (97 - 0)
    lo.interpolation_rows(97, 97)
    for m in (4, 8, 16):
        q = lo.QUIRK_MODULUS
        omega = lo.ROOTS_OF_UNITY[m]
        assert lo.domain(m, q) == [pow(omega, j, q) for j in range(m)]
        rng = np.random.default_rng(m)
        ev = [int(v) for v in rng.integers(0, q, size=m)]
        want = [0] * m
        for i in range(m):
            basis = lo.lagrange_basis_ntt(i, m, omega, q)
            want = [(w + ev[i] * c) % q for w, c in zip(want, basis)]
        assert lo.interpolate(ev, q) == want
    assert lo.domain(6, lo.QUIRK_MODULUS) == list(range(6))
    assert lo.domain(2, lo.QUIRK_MODULUS) == [0, 1]


# ---- honest proofs on the baseline path, CPU oracle commitment ----
def oracle_commit(oracle):
    return lambda msg, seed: oracle.lwe_commit(CQ, CN, CK, SIGMA, KEY_SEED, [v % CQ for v in msg], int(seed))


def honest_batch(oracle, m, q, batch, n_public, zk, seed=0):
    rng = np.random.default_rng(seed + m + 31 * zk)
    n, a, b, c = lo.random_circuit(rng, m, 4, q)
    rows_l = lo.interpolation_rows(m, q)
    publics, rows, proofs = [], [], []
    for i in range(batch):
        w = lo.extend_witness(rng.integers(0, 2**64, size=4, dtype=np.uint64), m, a, b, q)
        r = int(rng.integers(0, 2**64, dtype=np.uint64)) if zk else None
        row, proof, _, ln = lo.prove_one((a, b, c), m, q, w, n_public, oracle_commit(oracle), 1000 + i, r, rows_l)
        publics.append(w[:n_public]); rows.append(row); proofs.append(proof)
    return np.array(publics, dtype=np.uint64), np.array(rows, dtype=np.uint64), np.array(proofs, dtype=np.uint64)


@pytest.mark.parametrize("zk", [False, True])
@pytest.mark.parametrize("m,q", [(3, 97), (5, (1 << 31) - 1), (10, 17592186044423), (6, GOLD), (4, lo.QUIRK_MODULUS), (7, (1 << 44) + 1)])
def test_host_verify_mod_accepts_honest_proofs_and_rejects_the_tamper_matrix(pkg, oracle, m, q, zk):
    batch, n_public = 3, 2
    if q == lo.QUIRK_MODULUS:      # the omega domain: only all-zero evaluations prove — use a witness of zeros
        rng = np.random.default_rng(5)
        n, a, b, c = lo.random_circuit(rng, m, 4, q)
        w = np.zeros(n, dtype=np.uint64)
        row, proof, _, _ = lo.prove_one((a, b, c), m, q, w, n_public, oracle_commit(oracle), 77, 5 if zk else None)
        publics, rows, proofs = np.stack([w[:n_public]] * batch), np.stack([row] * batch), np.array([proof] * batch, dtype=np.uint64)
    else:
        publics, rows, proofs = honest_batch(oracle, m, q, batch, n_public, zk)
    assert list(pkg.verify_r1cs_batch(m, publics, rows, proofs, zk=zk, modulus=q)) == [1] * batch
    for w in range(13):
        for val in (None, q, q + 1 if q + 1 <= M64 else 0, M64):
            bad = proofs.copy()
            bad[1, w] = np.uint64(val) if val is not None else bad[1, w] ^ np.uint64(2)
            got = pkg.verify_r1cs_batch(m, publics, rows, bad, zk=zk, modulus=q)
            want = [lo.verify([int(v) for v in bad[i]], [int(v) for v in publics[i]], rows[i], m, q, zk) for i in range(batch)]
            assert list(got) == want, (w, val)
            assert got[0] == 1 and got[2] == 1
            if val is None and q != lo.QUIRK_MODULUS:              # (all-zero evaluations there: A B - C ignores a lone A or B)
                assert got[1] == (1 if (w == 12 and not zk) else 0), w      # plain mode ignores the blinding word
    bad_rows = rows.copy(); bad_rows[2, 1] ^= np.uint64(1)
    assert list(pkg.verify_r1cs_batch(m, publics, bad_rows, proofs, zk=zk, modulus=q)) == [1, 1, 0]


@pytest.mark.parametrize("zk", [False, True])
@pytest.mark.parametrize("m", [1, 2, 8])
def test_verify_mod_equals_verify_batch_on_the_ntt_path(pkg, m, zk):
    import test_r1cs_prove_abi as nttabi
    rng = np.random.default_rng(600 + m + zk)
    publics, rows, proofs = nttabi.honest_proofs(rng, m, 4, 2, 5, zk)
    proofs = np.concatenate([proofs, proofs]); rows = np.concatenate([rows, rows]); publics = np.concatenate([publics, publics])
    for i in range(4, 8):
        proofs[i, int(rng.integers(2, 13))] = np.uint64(int(rng.integers(0, 2**64, dtype=np.uint64)))
    want = pkg.verify_r1cs_batch(m, publics, rows, proofs, zk=zk)
    assert list(pkg.verify_r1cs_batch(m, publics, rows, proofs, zk=zk, modulus=GOLD)) == list(want)
    assert list(want[:4]) == [1] * 4
