"""Pure-Python restatement of the reference's witness-polynomial proofs (rust-api/lambda-snark/src/lib.rs prove_simple, prove_zk,
simulate_proof, verify_simple; opening.rs; polynomial.rs; challenge.rs) and of the two RNG crates they draw from, as pinned by the
reference's Cargo.lock: rand_core 0.6.4 (``SeedableRng::seed_from_u64``: PCG32 fills the 32-byte seed) and rand_chacha 0.3.1
(``ChaCha20Rng``: RFC 8439 ChaCha20, 64-bit block counter in words 12-13, stream 0 in words 14-15; ``next_u64`` = words 2j | 2j+1 << 32).
Written from those descriptions, independent of the library."""
import hashlib

import numpy as np

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1


def pcg32_seed(state):
    """``seed_from_u64``: the eight little-endian u32 key words."""
    words = []
    for _ in range(8):
        state = (state * 6364136223846793005 + 11634580027462260723) & M64
        xorshifted = (((state >> 18) ^ state) >> 27) & M32
        rot = state >> 59
        words.append(((xorshifted >> rot) | (xorshifted << ((32 - rot) & 31))) & M32)
    return words


def key_u64(words):
    """eight u32 key words -> four u64 words (the library's key layout)"""
    return [words[2 * i] | (words[2 * i + 1] << 32) for i in range(4)]


def _rotl(v, c):
    return ((v << c) | (v >> (32 - c))) & M32


def _quarter(x, a, b, c, d):
    x[a] = (x[a] + x[b]) & M32; x[d] = _rotl(x[d] ^ x[a], 16)
    x[c] = (x[c] + x[d]) & M32; x[b] = _rotl(x[b] ^ x[c], 12)
    x[a] = (x[a] + x[b]) & M32; x[d] = _rotl(x[d] ^ x[a], 8)
    x[c] = (x[c] + x[d]) & M32; x[b] = _rotl(x[b] ^ x[c], 7)


def chacha20_block(key_words, counter, nonce_words):
    """RFC 8439 §2.3: sixteen u32 output words for a key of eight u32 words, a 32-bit counter and a nonce of three u32 words."""
    init = [0x61707865, 0x3320646E, 0x79622D32, 0x6B206574] + list(key_words) + [counter & M32] + list(nonce_words)
    x = list(init)
    for _ in range(10):
        _quarter(x, 0, 4, 8, 12); _quarter(x, 1, 5, 9, 13); _quarter(x, 2, 6, 10, 14); _quarter(x, 3, 7, 11, 15)
        _quarter(x, 0, 5, 10, 15); _quarter(x, 1, 6, 11, 12); _quarter(x, 2, 7, 8, 13); _quarter(x, 3, 4, 9, 14)
    return [(x[i] + init[i]) & M32 for i in range(16)]


def chacha20rng_u64(key_words, count):
    """the first `count` ``next_u64`` draws of ``ChaCha20Rng::from_seed(key)`` (stream 0)"""
    out = []
    block = 0
    while len(out) < count:
        b = chacha20_block(key_words, block, [0, 0, 0])            # counter high word and the stream are 0
        out.extend(b[2 * j] | (b[2 * j + 1] << 32) for j in range(8))
        block += 1
    return out[:count]


def random_blinding(length, q, seed=None, key_words=None):
    """``Polynomial::random_blinding(length - 1, q, Some(seed))`` (or from a raw key)"""
    kw = pcg32_seed(seed) if key_words is None else key_words
    return [v % q for v in chacha20rng_u64(kw, length)]


def add_mod(a, b, q):
    s = a + b
    return s - q if s >= q else s


def from_witness(witness, q):
    return [int(w) % q for w in witness]


def evaluate(coeffs, alpha, q):
    """``Polynomial::evaluate``: Horner from the top coefficient, mul_mod then add_mod"""
    if not coeffs:
        return 0
    r = coeffs[-1]
    for c in reversed(coeffs[:-1]):
        r = add_mod(r * alpha % q, c, q)
    return r


def challenge_derive(public_inputs, words, q):
    """``Challenge::derive`` (challenge.rs:102-134) -> (alpha, hash32)"""
    h = hashlib.sha3_256()
    h.update(b"LAMBDA-SNARK-R-FS-v1")
    h.update(len(public_inputs).to_bytes(8, "little"))
    for v in public_inputs:
        h.update(int(v).to_bytes(8, "little"))
    h.update(len(words).to_bytes(8, "little"))
    h.update(np.asarray(words, dtype="<u8").tobytes())
    d = h.digest()
    return int.from_bytes(d[:8], "little") % q, d


def blinded(mode, q, length, witness=None, blinding_seed=None, key_words=None):
    """f' of prove_simple ("plain"), prove_zk ("zk") or simulate_proof ("simulate")"""
    if mode == "plain":
        return from_witness(witness, q)
    r = random_blinding(length, q, blinding_seed, key_words)
    if mode == "simulate":
        return r
    return [add_mod(f, b, q) for f, b in zip(from_witness(witness, q), r)]


def prove_one(mode, q, commit, public_inputs, seed, length, witness=None, blinding_seed=None, key_words=None):
    """-> (row, coeffs, [alpha, evaluation, seed], hash32).  commit(message, seed) returns the commitment words of
    ``Commitment::new(ctx, f', seed)`` (the words the transcript hashes)."""
    f = blinded(mode, q, length, witness, blinding_seed, key_words)
    row = commit(f, seed)
    alpha, h = challenge_derive(public_inputs, row, q)
    return row, f, [alpha, evaluate(f, alpha, q), int(seed)], h


def verify_one(q, public_inputs, words, proof, coeffs):
    """``verify_simple`` (lib.rs:1269-1285 + opening.rs:229-264)"""
    alpha, _ = challenge_derive(public_inputs, words, q)
    if int(proof[0]) != alpha:
        return 0
    if int(proof[1]) >= q or len(coeffs) == 0:
        return 0
    return 1 if evaluate([int(c) % q for c in coeffs], alpha, q) == int(proof[1]) else 0
