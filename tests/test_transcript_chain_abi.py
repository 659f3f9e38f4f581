"""CPU suite: the chained alpha -> beta transcript entry points and the kernel-choosing device call are declared, exported and
mirrored in ctypes; lsr_fs_challenge_chain_batch_flat equals hashlib's SHA3-256 over the transcript of challenge.rs:102-134 written
out here; the device forms refuse bad arguments (and a machine without a GPU) with -1; and the lane model of the
wavefront-cooperative Keccak (tools/experiments/sim_keccak_wave.py), gathering with the table it reads out of lsr_keccak_wave.hpp,
equals hashlib."""
import ctypes
import hashlib
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_H = os.path.join(ROOT, "include", "lambda_snark", "batch.h")
WAVE_HPP = os.path.join(ROOT, "lambda-snark-r_amd", "csrc", "lsr_keccak_wave.hpp")
SYMBOLS = {"lsr_fs_challenge_batch_device_on": 10, "lsr_fs_challenge_chain_batch_device": 12, "lsr_fs_challenge_chain_batch_flat": 11,
           "lsr_fs_transcript_path": 2}
AUTO, LANE, WAVE = 0, 1, 2
N_INPUTS = [0, 1, 2, 14, 15, 16, 17, 40]
ROW_WORDS = [1, 2, 13, 14, 15, 16, 17, 31, 33, 34, 100, 12293]
MODULI = [12289, 17592186044417, 2**64 - 2**32 + 1]


def derive(inputs, words, modulus):
    """challenge.rs:102-134: SHA3-256(tag || LE64(#inputs) || inputs || LE64(#words) || words); alpha = LE64(h[0..8]) mod q."""
    h = hashlib.sha3_256(b"LAMBDA-SNARK-R-FS-v1")
    h.update(len(inputs).to_bytes(8, "little"))
    h.update(np.asarray(inputs, dtype="<u8").tobytes())
    h.update(len(words).to_bytes(8, "little"))
    h.update(np.asarray(words, dtype="<u8").tobytes())
    digest = h.digest()
    return int.from_bytes(digest[:8], "little") % modulus, digest


def random_words(rng, shape, modulus):
    """64-bit words: some below the modulus, some at or above it, and the extremes."""
    w = rng.integers(0, 2**64, size=shape, dtype=np.uint64)
    flat = w.reshape(-1)
    flat[::5] %= np.uint64(modulus)
    if flat.size > 2:
        flat[1], flat[2] = np.uint64(2**64 - 1), np.uint64(modulus)
    return w


def sim():
    spec = importlib.util.spec_from_file_location("sim_keccak_wave", os.path.join(ROOT, "tools", "experiments", "sim_keccak_wave.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_declared_exported_and_mirrored(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(BATCH_H).read(), flags=re.S)
    lib = pkg._abi.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._abi.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name, n_args in SYMBOLS.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in exported and hasattr(lib, name), name
        assert len(pkg._abi.SIGNATURES[name][1]) == n_args, name
    m = re.search(r"enum\s*\{\s*LSR_FS_PATH_AUTO\s*=\s*0\s*,\s*LSR_FS_PATH_LANE\s*=\s*1\s*,\s*LSR_FS_PATH_WAVE\s*=\s*2\s*\}", text)
    assert m, "the path constants"


@pytest.mark.parametrize("row_words", ROW_WORDS)
def test_host_chain_matches_hashlib(lib, row_words):
    count = 5 if row_words > 1000 else 11
    for n_inputs in N_INPUTS:
        for mi, modulus in enumerate(MODULI):
            rng = np.random.default_rng(row_words * 1000 + n_inputs * 10 + mi)
            rows = random_words(rng, (count, row_words), modulus)
            ins = random_words(rng, (count, max(n_inputs, 1)), modulus)[:, :n_inputs].copy()
            want = []
            for i in range(count):
                a, ha = derive(ins[i], rows[i], modulus)
                b, hb = derive([a], rows[i], modulus)
                want.append((a, b, ha, hb))
            p_in = ins.ctypes.data if n_inputs else None
            for threads in (0, 1, 3):
                al = np.zeros(count, dtype=np.uint64); be = np.zeros(count, dtype=np.uint64)
                ha = np.zeros((count, 32), dtype=np.uint8); hb = np.zeros((count, 32), dtype=np.uint8)
                assert lib.lsr_fs_challenge_chain_batch_flat(p_in, n_inputs, rows.ctypes.data, row_words, count, modulus, al.ctypes.data, be.ctypes.data,
                                                             ha.ctypes.data, hb.ctypes.data, threads) == 0
                for i in range(count):
                    assert (int(al[i]), int(be[i]), bytes(ha[i]), bytes(hb[i])) == want[i], (row_words, n_inputs, modulus, threads, i)
            # equal to the two single calls, and the digests are optional (each on its own)
            a2 = np.zeros(count, dtype=np.uint64); b2 = np.zeros(count, dtype=np.uint64)
            h2a = np.zeros((count, 32), dtype=np.uint8); h2b = np.zeros((count, 32), dtype=np.uint8)
            assert lib.lsr_fs_challenge_batch_flat(p_in, n_inputs, rows.ctypes.data, row_words, count, modulus, a2.ctypes.data, h2a.ctypes.data, 2) == 0
            assert lib.lsr_fs_challenge_batch_flat(a2.ctypes.data, 1, rows.ctypes.data, row_words, count, modulus, b2.ctypes.data, h2b.ctypes.data, 2) == 0
            assert np.array_equal(a2, al) and np.array_equal(b2, be) and np.array_equal(h2a, ha) and np.array_equal(h2b, hb)
            a3 = np.zeros(count, dtype=np.uint64); b3 = np.zeros(count, dtype=np.uint64); h3 = np.zeros((count, 32), dtype=np.uint8)
            assert lib.lsr_fs_challenge_chain_batch_flat(p_in, n_inputs, rows.ctypes.data, row_words, count, modulus, a3.ctypes.data, b3.ctypes.data,
                                                         None, h3.ctypes.data, 2) == 0
            assert np.array_equal(a3, al) and np.array_equal(b3, be) and np.array_equal(h3, hb)
            assert lib.lsr_fs_challenge_chain_batch_flat(p_in, n_inputs, rows.ctypes.data, row_words, count, modulus, a3.ctypes.data, b3.ctypes.data,
                                                         None, None, 1) == 0
            assert np.array_equal(a3, al) and np.array_equal(b3, be)


def test_host_chain_argument_contract(lib):
    rows = np.arange(40, dtype=np.uint64); ins = np.arange(8, dtype=np.uint64)
    al = np.zeros(4, dtype=np.uint64); be = np.zeros(4, dtype=np.uint64)
    R, I, A, B = rows.ctypes.data, ins.ctypes.data, al.ctypes.data, be.ctypes.data
    f = lib.lsr_fs_challenge_chain_batch_flat
    assert f(I, 2, R, 10, 4, 12289, A, B, None, None, 0) == 0
    assert f(None, 2, R, 10, 4, 12289, A, B, None, None, 0) == -1      # null inputs with n_inputs > 0
    assert f(None, 0, None, 10, 4, 12289, A, B, None, None, 0) == -1    # null rows
    assert f(None, 0, R, 0, 4, 12289, A, B, None, None, 0) == -1        # empty rows
    assert f(None, 0, R, 10, 4, 0, A, B, None, None, 0) == -1           # zero modulus
    assert f(None, 0, R, 10, 4, 12289, None, B, None, None, 0) == -1    # null alphas
    assert f(None, 0, R, 10, 4, 12289, A, None, None, None, 0) == -1    # null betas
    al[:] = 77
    assert f(None, 0, R, 10, 0, 12289, A, B, None, None, 0) == 0 and (al == 77).all()   # count == 0 writes nothing


def test_device_argument_contract_needs_no_gpu(lib, pkg):
    """The checks come before any device work; with valid arguments and no GPU the launch fails: -1 and a message, never a crash."""
    buf = np.zeros(64, dtype=np.uint64)
    P = buf.ctypes.data      # a host pointer: refused calls never touch it, and without a GPU no kernel runs
    single, chain = lib.lsr_fs_challenge_batch_device_on, lib.lsr_fs_challenge_chain_batch_device
    for path in (AUTO, LANE, WAVE):
        assert single(path, None, 2, P, 4, 2, 12289, P, None, None) == -1
        assert single(path, None, 0, None, 4, 2, 12289, P, None, None) == -1
        assert single(path, None, 0, P, 0, 2, 12289, P, None, None) == -1
        assert single(path, None, 0, P, 4, 2, 0, P, None, None) == -1
        assert single(path, None, 0, P, 4, 2, 12289, None, None, None) == -1
        assert single(path, None, 0, P, 4, 0, 12289, P, None, None) == 0
        assert chain(path, None, 2, P, 4, 2, 12289, P, P, None, None, None) == -1
        assert chain(path, None, 0, None, 4, 2, 12289, P, P, None, None, None) == -1
        assert chain(path, None, 0, P, 0, 2, 12289, P, P, None, None, None) == -1
        assert chain(path, None, 0, P, 4, 2, 0, P, P, None, None, None) == -1
        assert chain(path, None, 0, P, 4, 2, 12289, None, P, None, None, None) == -1
        assert chain(path, None, 0, P, 4, 2, 12289, P, None, None, None, None) == -1
        assert chain(path, None, 0, P, 4, 0, 12289, P, P, None, None, None) == 0
    for path in (3, -1, 99):
        assert single(path, None, 0, P, 4, 2, 12289, P, None, None) == -1
        assert "path" in pkg._abi.last_error()
        assert chain(path, None, 0, P, 4, 2, 12289, P, P, None, None, None) == -1
        assert "path" in pkg._abi.last_error()
        assert chain(path, None, 0, P, 4, 0, 12289, P, P, None, None, None) == -1     # also with nothing to do
    if lib.lsr_device_count() == 0:
        for path in (AUTO, LANE, WAVE):
            assert single(path, None, 0, P, 4, 2, 12289, P + 256, None, None) == -1
            assert pkg._abi.last_error()
            assert chain(path, None, 0, P, 4, 2, 12289, P + 256, P + 384, None, None, None) == -1
            assert pkg._abi.last_error()


def test_transcript_path_answers_without_a_device(lib):
    f = lib.lsr_fs_transcript_path
    picks = [f(c, 12293) for c in (0, 1, 2, 64, 4096, 2**20, 2**40)]
    assert set(picks) <= {LANE, WAVE}
    assert picks[1] == WAVE and picks[-1] == LANE, "small batches go to the wave kernel, huge ones to the lane kernel"
    switched = [i for i in range(1, len(picks)) if picks[i] != picks[i - 1]]
    assert len(switched) == 1, "one switch point"
    assert f(1, 1) in (LANE, WAVE) and f(1, 2**30) in (LANE, WAVE)


def test_lane_model_reads_the_kernels_table_and_equals_hashlib():
    m = sim()
    assert os.path.samefile(m.HEADER, WAVE_HPP)
    text = open(WAVE_HPP).read()
    # the kernel's table is the literal the model parses, and there is one of it
    assert text.count("LSR_KECCAK_WAVE_TABLE_BEGIN") == 1 and text.count("LSR_KECCAK_WAVE_TABLE_END") == 1
    body = text[text.index("LSR_KECCAK_WAVE_TABLE_BEGIN"):text.index("LSR_KECCAK_WAVE_TABLE_END")]
    assert "kKeccakWaveTable[32][16]" in body and "kKeccakWaveTable[lane & 31]" in text
    table = m.header_table()
    assert table == m.derive_table()
    assert m.check(messages=120, seed=5) >= 100
    # a wrong table is noticed: swap two chi sources
    bad = [row[:] for row in table]
    bad[7][6], bad[7][7] = bad[7][7], bad[7][6]
    got = m.WaveModel(bad).sha3_256_pair(b"abc", b"")
    assert got[0] != hashlib.sha3_256(b"abc").digest()
    good = m.WaveModel(table).sha3_256_pair(b"abc", b"")
    assert good == [hashlib.sha3_256(b"abc").digest(), hashlib.sha3_256(b"").digest()]
