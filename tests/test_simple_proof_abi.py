"""CPU suite: the witness-polynomial proof calls of prover.h that need no GPU — ChaCha20Rng keys and
random_blinding against tests/simple_oracle.py, verify_simple on oracle-built proofs, and argument checks."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simple_oracle as so  # noqa: E402

GOLD = 18446744069414584321
P44 = (1 << 44) + 1
MODULI = [P44, 17592169062401, GOLD, 97, 3, (1 << 64) - 59]
SEEDS = [0, 1, 42, (1 << 64) - 1]
LENGTHS = [1, 7, 8, 9, 4097]


def test_oracle_chacha_block_reproduces_rfc8439(golden_dir):
    v = json.load(open(os.path.join(golden_dir, "rfc8439_chacha20.json")))
    kb, nb = bytes.fromhex(v["key_bytes_hex"]), bytes.fromhex(v["nonce_bytes_hex"])
    key = [int.from_bytes(kb[4 * i:4 * i + 4], "little") for i in range(8)]
    nonce = [int.from_bytes(nb[4 * i:4 * i + 4], "little") for i in range(3)]
    assert so.chacha20_block(key, v["counter"], nonce) == [int(w, 16) for w in v["output_words_hex"]]
    assert so.chacha20rng_u64([0] * 8, 2) == [0x903DF1A0ADE0B876, 0x28BD8653E56A5D40]   # RFC 8439 A.1 #1, zero key


def test_symbols_and_signatures(pkg):
    for name in ("lsr_chacha20rng_keys_from_u64", "lsr_random_blinding", "lsr_random_blinding_device", "lsr_simple_prover_create",
                 "lsr_simple_prover_free", "lsr_simple_prover_modulus", "lsr_simple_prove_batch", "lsr_simple_prove_batch_device",
                 "lsr_simple_verify_batch", "lsr_simple_verify_batch_device"):
        assert name in pkg._abi.SIGNATURES
    assert pkg.SIMPLE_PROOF_WORDS == 3 and pkg.SIMPLE_MODES == {"plain": 0, "zk": 1, "simulate": 2}


def test_keys_from_u64_match_pcg32(pkg):
    keys = pkg.chacha20rng_keys(np.array(SEEDS, dtype=np.uint64))
    for s, k in zip(SEEDS, keys):
        assert [int(v) for v in k] == so.key_u64(so.pcg32_seed(s))


def test_random_blinding_matches_the_oracle(pkg):
    keys = pkg.chacha20rng_keys(np.array(SEEDS, dtype=np.uint64))
    draws = [so.chacha20rng_u64(so.pcg32_seed(s), max(LENGTHS)) for s in SEEDS]
    for q in MODULI:
        for length in LENGTHS:
            out = pkg.random_blinding(keys, length, q)
            assert out.shape == (len(SEEDS), length)
            for i in range(len(SEEDS)):
                assert [int(v) for v in out[i]] == [d % q for d in draws[i][:length]], (q, length, SEEDS[i])
    zero = pkg.random_blinding(np.zeros((1, 4), dtype=np.uint64), 2, GOLD)      # raw zero key: the RFC 8439 A.1 keystream
    assert [int(v) for v in zero[0]] == [0x903DF1A0ADE0B876 % GOLD, 0x28BD8653E56A5D40 % GOLD]


def test_random_blinding_refuses_even_or_tiny_moduli(pkg):
    keys = pkg.chacha20rng_keys([1])
    for q in (0, 1, 2, 4, 1 << 44):
        with pytest.raises(pkg.CoreError, match="odd"):
            pkg.random_blinding(keys, 4, q)


def test_polynomial_doc_values():
    assert so.evaluate(so.from_witness([1, 7, 13, 91], 17592186044417), 2, 17592186044417) == 795   # polynomial.rs:85-95
    assert so.evaluate([], 5, 97) == 0


def fake_proofs(rng, q, batch, length, n_public, words=40):
    """proofs that verify_simple accepts, built by the oracle over arbitrary commitment words (verify_simple does not open them)"""
    rows = rng.integers(0, 2**63, size=(batch, words), dtype=np.uint64)
    pub = rng.integers(0, 2**64, size=(batch, n_public), dtype=np.uint64)
    coeffs = rng.integers(0, 2**64, size=(batch, length), dtype=np.uint64)     # raw words: verify reduces them mod q
    proofs = np.zeros((batch, 3), dtype=np.uint64)
    for i in range(batch):
        alpha, _ = so.challenge_derive([int(v) for v in pub[i]], rows[i], q)
        proofs[i] = [alpha, so.evaluate([int(c) % q for c in coeffs[i]], alpha, q), i + 1]
    return pub, rows, proofs, coeffs


@pytest.mark.parametrize("q", [P44, 17592169062401, GOLD, 97])
@pytest.mark.parametrize("length", [1, 4, 65, 300])
@pytest.mark.parametrize("n_public", [0, 2])
def test_host_verify_accepts_and_rejects_each_tampering(pkg, q, length, n_public):
    rng = np.random.default_rng(length * 7 + n_public + q % 1000)
    batch = 3
    pub, rows, proofs, coeffs = fake_proofs(rng, q, batch, length, n_public)
    assert list(pkg.verify_simple_batch(q, pub, rows, proofs, coeffs)) == [1] * batch
    cases = []
    p = proofs.copy(); p[0, 0] ^= np.uint64(1); cases.append((pub, rows, p, coeffs, 0))                          # alpha
    p = proofs.copy(); p[1, 0] = np.uint64(int(p[1, 0]) + q) if int(p[1, 0]) + q < 2**64 else p[1, 0] ^ np.uint64(4)
    cases.append((pub, rows, p, coeffs, 1))                                                                      # alpha + q (raw compare)
    p = proofs.copy(); p[2, 1] = np.uint64((int(p[2, 1]) + 1) % q); cases.append((pub, rows, p, coeffs, 2))       # evaluation
    p = proofs.copy(); p[0, 1] = np.uint64(q); cases.append((pub, rows, p, coeffs, 0))                            # evaluation = q
    p = proofs.copy(); p[1, 1] = np.uint64(int(p[1, 1]) + q) if int(p[1, 1]) + q < 2**64 else np.uint64(2**64 - 1)
    cases.append((pub, rows, p, coeffs, 1))                                                                      # evaluation + q
    c = coeffs.copy(); c[2, length // 2] ^= np.uint64(1); cases.append((pub, rows, proofs, c, 2))                 # one coefficient
    r = rows.copy(); r[1, 5] ^= np.uint64(1); cases.append((pub, r, proofs, coeffs, 1))                           # one row word
    if n_public:
        u = pub.copy(); u[0, 1] ^= np.uint64(1); cases.append((u, rows, proofs, coeffs, 0))                       # one public input
    for pu, ro, pr, co, bad in cases:
        got = pkg.verify_simple_batch(q, pu, ro, pr, co)
        want = [so.verify_one(q, [int(v) for v in pu[i]], ro[i], pr[i], [int(v) for v in co[i]]) for i in range(batch)]
        assert list(got) == want
        assert got[bad] == 0 and sum(got) == batch - 1
    p = proofs.copy(); p[:, 2] = 0                                                                               # the seed word is not checked
    assert list(pkg.verify_simple_batch(q, pub, rows, p, coeffs)) == [1] * batch


def test_host_verify_rejects_an_empty_opening(pkg):
    q = P44
    rng = np.random.default_rng(5)
    rows = rng.integers(0, 2**63, size=(2, 16), dtype=np.uint64)
    pub = np.zeros((2, 0), dtype=np.uint64)
    proofs = np.array([[so.challenge_derive([], rows[i], q)[0], 0, 1] for i in range(2)], dtype=np.uint64)
    assert list(pkg.verify_simple_batch(q, pub, rows, proofs, np.zeros((2, 0), dtype=np.uint64))) == [0, 0]


def test_argument_checks(pkg):
    lib = pkg._abi.load_library()
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.addressof(buf)
    res = (ctypes.c_int * 4)()
    r = ctypes.addressof(res)
    fake = ctypes.addressof((ctypes.c_uint64 * 64)())   # never dereferenced: the checks come first
    for q in (0, 1, 2, 4, 1 << 44):
        assert lib.lsr_simple_verify_batch(q, p, 1, p, 4, p, p, 2, 1, None, 0, r) == -1 and "odd" in pkg._abi.last_error()
        assert lib.lsr_simple_verify_batch_device(q, p, 1, p, 4, p, p, 2, 1, None, 0, r, None) == -1
        assert lib.lsr_random_blinding_device(p, 1, 4, q, p, None) == -1
        assert lib.lsr_simple_prover_create(q, -1) is None and "odd" in pkg._abi.last_error()
    for args in ([P44, None, 1, p, 4, p, p, 2, 1, None, 0, r], [P44, p, 1, None, 4, p, p, 2, 1, None, 0, r],
                 [P44, p, 1, p, 4, None, p, 2, 1, None, 0, r], [P44, p, 1, p, 4, p, None, 2, 1, None, 0, r],
                 [P44, p, 1, p, 4, p, p, 2, 1, None, 0, None]):
        assert lib.lsr_simple_verify_batch(*args) == -1 and "NULL" in pkg._abi.last_error()
        assert lib.lsr_simple_verify_batch_device(*(args + [None])) == -1
    assert lib.lsr_simple_verify_batch(P44, p, 1, p, 0, p, p, 2, 1, None, 0, r) == -1           # words_per_row 0
    assert lib.lsr_simple_verify_batch(P44, p, 1, p, 4, p, p, 2, 0, None, 0, r) == 0            # batch 0
    assert lib.lsr_chacha20rng_keys_from_u64(None, 1, p) == -1 and lib.lsr_chacha20rng_keys_from_u64(p, 1, None) == -1
    assert lib.lsr_random_blinding(None, 1, 4, P44, p) == -1 and lib.lsr_random_blinding(p, 1, 4, P44, None) == -1
    for dev in (False, True):
        fn = lib.lsr_simple_prove_batch_device if dev else lib.lsr_simple_prove_batch
        extra = [None] if dev else []
        base = [fake, fake, P44, 0, p, 4, 1, p, 1, p, p, p, p, p, None]
        for idx, why in ((0, "NULL"), (1, "NULL"), (4, "NULL"), (7, "NULL"), (9, "NULL"), (11, "NULL"), (12, "NULL"), (13, "NULL")):
            args = list(base); args[idx] = None
            assert fn(*(args + extra)) == -1 and why in pkg._abi.last_error(), idx
        for mode in (-1, 3, 7):
            args = list(base); args[3] = mode
            assert fn(*(args + extra)) == -1 and "mode" in pkg._abi.last_error()
        args = list(base); args[5] = 0
        assert fn(*(args + extra)) == -1 and "empty" in pkg._abi.last_error()
