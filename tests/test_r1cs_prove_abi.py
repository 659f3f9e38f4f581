"""CPU suite: the batched prove_r1cs / verify_r1cs entry points (include/lambda_snark/prover.h) are declared, exported and mirrored,
their argument checks answer -1 before any device work, and the host verifier — which needs no GPU — accepts honest proofs built
here from the oracle, rejects every tampered word, and agrees with a restatement of verify_r1cs[_zk] (lib.rs:1016-1095, 1142-1215)
for any 64-bit proof word."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROVER_H = os.path.join(ROOT, "include", "lambda_snark", "prover.h")
SYMBOLS = ["lsr_r1cs_prove_batch", "lsr_r1cs_prove_batch_device", "lsr_r1cs_verify_batch", "lsr_r1cs_verify_batch_device",
           "lsr_prover_eval_batch_device"]
Q = 18446744069414584321
M64 = (1 << 64) - 1
ALPHA, BETA, Q_ALPHA, Q_BETA, A_ALPHA, B_ALPHA, C_ALPHA, A_BETA, B_BETA, C_BETA, OPEN_ALPHA, OPEN_BETA, BLINDING = range(13)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prover_replay  # noqa: E402


def test_prover_h_declares_the_prove_and_verify_calls():
    text = re.sub(r"/\*.*?\*/", "", open(PROVER_H).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
    assert "LSR_R1CS_PROOF_WORDS" in text and "LSR_PROOF_BLINDING" in text


def test_library_exports_and_signatures(pkg):
    lib = pkg._abi.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in pkg._abi.SIGNATURES, name
    assert len(pkg._abi.SIGNATURES["lsr_r1cs_prove_batch"][1]) == 12
    assert len(pkg._abi.SIGNATURES["lsr_r1cs_prove_batch_device"][1]) == 13
    assert len(pkg._abi.SIGNATURES["lsr_r1cs_verify_batch"][1]) == 9
    assert len(pkg._abi.SIGNATURES["lsr_r1cs_verify_batch_device"][1]) == 10
    assert len(pkg._abi.SIGNATURES["lsr_prover_eval_batch_device"][1]) == 7
    assert hasattr(pkg.R1csProver, "prove_batch") and hasattr(pkg.R1csProver, "prove_batch_device")
    assert callable(pkg.verify_r1cs_batch) and callable(pkg.prover_eval_batch_device) and pkg.PROOF_WORDS == 13


@pytest.mark.parametrize("device", [False, True])
def test_prove_null_arguments_are_refused(pkg, device):
    lib = pkg._abi.load_library()
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.addressof(buf)
    fake = ctypes.addressof((ctypes.c_uint64 * 64)())   # never dereferenced: NULL checks come first
    fn = lib.lsr_r1cs_prove_batch_device if device else lib.lsr_r1cs_prove_batch
    cases = [(None, fake, p, p, p, p, p), (fake, None, p, p, p, p, p), (fake, fake, None, p, p, p, p), (fake, fake, p, None, p, p, p),
             (fake, fake, p, p, None, p, p), (fake, fake, p, p, p, None, p), (fake, fake, p, p, p, p, None)]
    for prover, lwe, w, seeds, rows, proofs, status in cases:
        args = [prover, lwe, 17592186044417, w, 1, 0, seeds, None, rows, proofs, None, status]
        rc = fn(*(args + [None] if device else args))
        assert rc == -1
        assert "NULL" in pkg._abi.last_error()


@pytest.mark.parametrize("device", [False, True])
def test_verify_argument_checks(pkg, device):
    lib = pkg._abi.load_library()
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.addressof(buf)
    res = (ctypes.c_int * 4)()
    r = ctypes.addressof(res)
    fn = lib.lsr_r1cs_verify_batch_device if device else lib.lsr_r1cs_verify_batch
    extra = [None] if device else []
    for args in ([4, None, 1, p, 4, p, 1, 0, r], [4, p, 1, None, 4, p, 1, 0, r], [4, p, 1, p, 4, None, 1, 0, r], [4, p, 1, p, 4, p, 1, 0, None]):
        assert fn(*(args + extra)) == -1 and "NULL" in pkg._abi.last_error()
    for m in (0, 3, 6, 100):
        assert fn(*([m, p, 1, p, 4, p, 1, 0, r] + extra)) == -1 and "power of two" in pkg._abi.last_error()
    assert fn(*([4, p, 1, p, 0, p, 1, 0, r] + extra)) == -1
    assert fn(*([4, p, 1, p, 4, p, 0, 0, r] + extra)) == 0        # batch 0


def test_eval_argument_checks(pkg):
    lib = pkg._abi.load_library()
    p = ctypes.addressof((ctypes.c_uint64 * 8)())
    assert lib.lsr_prover_eval_batch_device(None, 4, 1, p, 1, p, None) == -1
    assert lib.lsr_prover_eval_batch_device(p, 4, 1, None, 1, p, None) == -1
    assert lib.lsr_prover_eval_batch_device(p, 4, 1, p, 1, None, None) == -1
    assert lib.lsr_prover_eval_batch_device(p, 0, 1, p, 1, p, None) == -1
    assert lib.lsr_prover_eval_batch_device(p, 4, 1, p, 0, p, None) == -1


# ---- a restatement of verify_r1cs / verify_r1cs_zk with arith.rs's u64 / u128 semantics (wrapping u128 like Rust release builds) ----
def _mul_mod(a, b):
    return (a * b) % Q


def _sub_mod(a, b):
    d = (a + Q - b) % (1 << 128)
    if d >= Q:
        d = (d - Q) % (1 << 128)
    return d & M64


def _zh(x, m):
    return _sub_mod(pow(x % Q, m, Q), 1)


def restated_verify(proof, public, row, m, zk):
    alpha, _ = prover_replay.challenge_derive(public, row, Q)
    if proof[ALPHA] != alpha:
        return 0
    beta, _ = prover_replay.challenge_derive([proof[ALPHA]], row, Q)
    if proof[BETA] != beta:
        return 0
    for k, x in ((0, proof[ALPHA]), (1, proof[BETA])):
        zh = _zh(x, m)
        q = proof[Q_ALPHA + k]
        if zk:
            q = _sub_mod(q, _mul_mod(proof[BLINDING], zh))
        lhs = _mul_mod(q, zh)
        rhs = _sub_mod(_mul_mod(proof[A_ALPHA + 3 * k], proof[B_ALPHA + 3 * k]), proof[C_ALPHA + 3 * k])
        if lhs != rhs:
            return 0
    return int(proof[OPEN_ALPHA] == proof[Q_ALPHA] and proof[OPEN_BETA] == proof[Q_BETA])


def honest_proofs(rng, m, batch, n_public, words, zk):
    """proofs built from random A, B evaluations on H with c = a b (so Q exists): interpolants and Q by exact Python arithmetic"""
    omega = pow(7, (Q - 1) // m, Q) if m > 1 else 1
    publics = rng.integers(0, 2**64, size=(batch, n_public), dtype=np.uint64)
    rows = rng.integers(0, 2**64, size=(batch, words), dtype=np.uint64)
    proofs = np.zeros((batch, 13), dtype=np.uint64)
    m_inv = pow(m, -1, Q)
    for i in range(batch):
        a = [int(v) for v in rng.integers(0, Q, size=m, dtype=np.uint64)]
        b = [int(v) for v in rng.integers(0, Q, size=m, dtype=np.uint64)]
        c = [x * y % Q for x, y in zip(a, b)]
        interp = lambda ev: [m_inv * sum(ev[k] * pow(omega, (Q - 1 - j * k % (Q - 1)) % (Q - 1), Q) for k in range(m)) % Q for j in range(m)]
        pa, pb, pc = interp(a), interp(b), interp(c)
        prod = [0] * (2 * m - 1)
        for s, x in enumerate(pa):
            for t, y in enumerate(pb):
                prod[s + t] = (prod[s + t] + x * y) % Q
        num = [(prod[j] - (pc[j] if j < m else 0)) % Q for j in range(2 * m - 1)]
        quot = [0] * max(1, m - 1)
        for j in range(2 * m - 2, m - 1, -1):          # divide by X^m - 1
            quot[j - m] = num[j]
            num[j - m] = (num[j - m] + num[j]) % Q
            num[j] = 0
        assert not any(num)
        r = int(rng.integers(0, 2**64, dtype=np.uint64)) if zk else 0
        alpha, _ = prover_replay.challenge_derive([int(v) for v in publics[i]], rows[i], Q)
        beta, _ = prover_replay.challenge_derive([alpha], rows[i], Q)
        ev = lambda poly, x: prover_replay.eval_poly(poly, x, Q)
        qa, qb = ev(quot, alpha), ev(quot, beta)
        if zk:
            qa = (qa + (r % Q) * (pow(alpha, m, Q) - 1)) % Q
            qb = (qb + (r % Q) * (pow(beta, m, Q) - 1)) % Q
        proofs[i] = [alpha, beta, qa, qb, ev(pa, alpha), ev(pb, alpha), ev(pc, alpha), ev(pa, beta), ev(pb, beta), ev(pc, beta), qa, qb, r % Q]
    return publics, rows, proofs


@pytest.mark.parametrize("zk", [False, True])
@pytest.mark.parametrize("m", [1, 2, 8])
def test_host_verify_accepts_honest_proofs_and_rejects_each_tampered_word(pkg, m, zk):
    rng = np.random.default_rng(90 + m + 7 * zk)
    batch, n_public, words = 4, 3, 9
    publics, rows, proofs = honest_proofs(rng, m, batch, n_public, words, zk)
    assert list(pkg.verify_r1cs_batch(m, publics, rows, proofs, zk=zk)) == [1] * batch
    for w in range(13):
        bad = proofs.copy()
        bad[2, w] ^= np.uint64(1 << 5)
        expect = [1, 1, 1 if (w == BLINDING and not zk) else 0, 1]      # plain mode ignores the blinding word
        assert list(pkg.verify_r1cs_batch(m, publics, rows, bad, zk=zk)) == expect, w
    bad_rows = rows.copy(); bad_rows[1, 4] ^= np.uint64(1)
    assert list(pkg.verify_r1cs_batch(m, publics, bad_rows, proofs, zk=zk)) == [1, 0, 1, 1]
    bad_pub = publics.copy(); bad_pub[3, 0] ^= np.uint64(1)
    assert list(pkg.verify_r1cs_batch(m, bad_pub, rows, proofs, zk=zk)) == [1, 1, 1, 0]


@pytest.mark.parametrize("zk", [False, True])
def test_host_verify_agrees_with_the_restatement_on_wide_words(pkg, zk):
    """proof words >= p and near 2^64 go through add/sub/mul_mod exactly as the Rust code would take them"""
    rng = np.random.default_rng(77 + zk)
    m, batch, n_public, words = 4, 40, 2, 6
    publics, rows, proofs = honest_proofs(rng, m, 4, n_public, words, zk)
    publics = np.concatenate([publics] * 10); rows = np.concatenate([rows] * 10); proofs = np.concatenate([proofs] * 10)
    wide = [Q, Q + 1, M64, M64 - 1, Q - 1, 0, 1 << 63]
    for i in range(4, batch):
        for w in range(2, 13):
            if rng.random() < 0.4:
                proofs[i, w] = np.uint64(wide[int(rng.integers(0, len(wide)))] if rng.random() < 0.7 else (int(proofs[i, w]) + Q) & M64)
    # a family that still verifies: Q word + p in zk is unblinded by sub_mod; A + p keeps mul_mod's residue
    proofs[5, A_ALPHA] = np.uint64(int(proofs[1, A_ALPHA]) + Q) if int(proofs[1, A_ALPHA]) + Q <= M64 else proofs[1, A_ALPHA]
    got = pkg.verify_r1cs_batch(m, publics, rows, proofs, zk=zk)
    want = [restated_verify([int(v) for v in proofs[i]], [int(v) for v in publics[i]], rows[i], m, zk) for i in range(batch)]
    assert list(got) == want
    assert sum(want[:4]) == 4
