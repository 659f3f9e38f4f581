"""Python-integer model of the bit-packed ring elements (batch.h "bit-packed ring elements"), written from the
definition in batch.h and not from the kernels, with its own tests (collected by test_ring_pack_abi.py).

Everything here is exact Python-integer arithmetic on lists; `pack_array` / `unpack_array` wrap it for numpy batches."""
import numpy as np
import pytest

CENTRED, RESIDUE = 0, 1
Q44 = 17592169062401
GOLDILOCKS = 2**64 - 2**32 + 1


def words(n, bits):
    return -(-n * bits // 64) if 1 <= bits <= 63 else 0


def min_bits(q, mode, bound):
    if bound == 0 or mode not in (CENTRED, RESIDUE):
        return 0
    if mode == CENTRED:
        if bound > (q - 1) // 2:
            return 0
        bits = bound.bit_length() + 1
    else:
        if bound > q - 1:
            return 0
        bits = bound.bit_length()
    return bits if bits <= 63 else 0


def centre(x, q):
    return x if x <= (q - 1) // 2 else x - q


def field_range(mode, bits):
    """(lowest, highest) value in range"""
    return (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if mode == CENTRED else (0, (1 << bits) - 1)


BLOCK = 256     # fields joined or split at a time: Python integers of n bits fields cost n bits per shift, so long elements go in two levels


def _join(fields, bits):
    """sum of fields[i] << (i bits)"""
    blocks = [sum(f << (i * bits) for i, f in enumerate(fields[k:k + BLOCK])) for k in range(0, len(fields), BLOCK)]
    return sum(b << (k * BLOCK * bits) for k, b in enumerate(blocks))


def _split(stream, n, bits):
    """[(stream >> (i bits)) mod 2^bits for i < n]"""
    fields = []
    for k in range(0, n, BLOCK):
        block = (stream >> (k * bits)) & ((1 << (BLOCK * bits)) - 1)
        fields += [(block >> (i * bits)) & ((1 << bits) - 1) for i in range(min(BLOCK, n - k))]
    return fields


def pack(x, q, bits, mode):
    """one element: (words, status)"""
    n = len(x)
    status, fields = 1, []
    lo, hi = field_range(mode, bits)
    for w in x:
        w = int(w)
        if w >= q:
            status, v = -1, w
        else:
            v = centre(w, q) if mode == CENTRED else w
            if not lo <= v <= hi and status == 1:
                status = 0
        fields.append(v % (1 << bits))
    stream = _join(fields, bits)
    raw = stream.to_bytes(8 * words(n, bits), "little")      # word k is bits 64 k .. 64 k + 63
    return [int.from_bytes(raw[8 * k:8 * k + 8], "little") for k in range(words(n, bits))], status


def unpack(w, n, q, bits, mode):
    """one element: (coefficients, status)"""
    assert len(w) == words(n, bits)
    stream = int.from_bytes(b"".join(int(v).to_bytes(8, "little") for v in w), "little")
    status, out = 1, []
    half = (q - 1) // 2
    for f in _split(stream, n, bits):
        if mode == CENTRED:
            v = f - (1 << bits) if f >> (bits - 1) else f
            ok, word = abs(v) <= half, v % q
        else:
            ok, word = f < q, f
        if not ok:
            status, word = 0, 0
        out.append(word)
    if stream >> (n * bits):
        status = 0
    return out, status


def pack_array(x, q, bits, mode):
    x = np.asarray(x, dtype=np.uint64)
    rows = [pack(row.tolist(), q, bits, mode) for row in x.reshape(-1, x.shape[-1])]
    return np.array([r[0] for r in rows], dtype=np.uint64).reshape(len(rows), -1), np.array([r[1] for r in rows], dtype=np.int32)


def unpack_array(w, n, q, bits, mode):
    w = np.asarray(w, dtype=np.uint64)
    rows = [unpack(row.tolist(), n, q, bits, mode) for row in w.reshape(-1, w.shape[-1])]
    return np.array([r[0] for r in rows], dtype=np.uint64).reshape(len(rows), n), np.array([r[1] for r in rows], dtype=np.int32)


def admits(q, mode, bits):
    """`bits` whose whole range is valid under q: every in-range value round-trips"""
    return (1 << (bits - 1)) <= (q - 1) // 2 if mode == CENTRED else (1 << bits) <= q


def in_range_element(rng, n, q, bits, mode):
    """n random in-range canonical words with the range's two end values in the first and the last coefficient"""
    lo, hi = field_range(mode, bits)
    half = (q - 1) // 2
    lo, hi = (max(lo, -half), min(hi, half)) if mode == CENTRED else (0, min(hi, q - 1))
    v = [lo + int(rng.integers(0, 2**63)) % (hi - lo + 1) for _ in range(n)]
    v[0], v[-1] = lo, hi
    return [a % q for a in v]


# ---- the model's own tests -----------------------------------------------------------------------------------------------------------------
def test_by_hand_vector_packs_to_0x8f9():
    q = Q44
    assert pack([1, q - 1, 3, q - 4], q, 3, CENTRED) == ([0x8F9], 1)
    assert pack([1, q - 1, 4, q - 4], q, 3, CENTRED)[1] == 0
    assert pack([1, q - 1, 4, q - 4], q, 3, CENTRED)[0] == [0x8F9 ^ (3 << 6) ^ (4 << 6)]      # the field is truncated: 4 mod 8
    assert pack([1, q, 4, q - 4], q, 3, CENTRED)[1] == -1                                      # a word >= q outranks the range
    assert unpack([0x8F9], 4, q, 3, CENTRED) == ([1, q - 1, 3, q - 4], 1)


@pytest.mark.parametrize("mode", [CENTRED, RESIDUE])
@pytest.mark.parametrize("bits", [1, 2, 3, 7, 11, 13, 31, 32, 33, 44, 45, 63])
def test_round_trips_with_the_end_values(bits, mode):
    rng = np.random.default_rng(bits * 2 + mode)
    for q in (Q44, GOLDILOCKS):
        for n in (2, 4, 16, 64, 128, 4096):
            x = in_range_element(rng, n, q, bits, mode)
            w, status = pack(x, q, bits, mode)
            assert status == 1 and len(w) == words(n, bits)
            assert unpack(w, n, q, bits, mode) == (x, 1)
            assert pack(unpack(w, n, q, bits, mode)[0], q, bits, mode) == (w, 1)
            if n * bits % 64:
                assert w[-1] >> (n * bits % 64) == 0


def test_the_three_invalid_decodes():
    q = 12289
    half = (q - 1) // 2
    # a CENTRED field beyond (q - 1) / 2, on either side: the word is 0, the others stand
    for v in (half + 1, -half - 1):
        w = [(v % (1 << 15)) << 15 | 5]
        assert unpack(w + [0] * (words(64, 15) - 1), 64, q, 15, CENTRED) == ([5, 0] + [0] * 62, 0)
    assert unpack([(half % (1 << 15)) << 15 | 5] + [0] * 14, 64, q, 15, CENTRED) == ([5, half] + [0] * 62, 1)
    assert unpack([((-half) % (1 << 15)) << 15 | 5] + [0] * 14, 64, q, 15, CENTRED) == ([5, q - half] + [0] * 62, 1)
    # a RESIDUE field >= q
    assert unpack([q << 14 | 7] + [0] * 13, 64, q, 14, RESIDUE) == ([7, 0] + [0] * 62, 0)
    assert unpack([(q - 1) << 14 | 7] + [0] * 13, 64, q, 14, RESIDUE) == ([7, q - 1] + [0] * 62, 1)
    # a non-zero padding bit at n = 2, bits = 3: the fields decode, the status is 0
    assert unpack([0b001_010], 2, q, 3, CENTRED) == ([2, 1], 1)
    assert unpack([0b1_001_010], 2, q, 3, CENTRED) == ([2, 1], 0)
    assert unpack([1 << 63 | 0b001_010], 2, q, 3, RESIDUE) == ([2, 1], 0)


def test_words_and_min_bits():
    assert [words(n, b) for n, b in [(2, 3), (64, 11), (16, 4), (16, 5), (4096, 63), (2, 0), (2, 64)]] == [1, 11, 1, 2, 4032, 0, 0]
    assert [min_bits(Q44, CENTRED, b) for b in (0, 1, 2, 1023, 1024, (Q44 - 1) // 2, (Q44 - 1) // 2 + 1)] == [0, 2, 3, 11, 12, 44, 0]
    assert [min_bits(Q44, RESIDUE, b) for b in (0, 1, 2, 1023, 1024, Q44 - 1, Q44)] == [0, 1, 2, 10, 11, 44, 0]
    assert min_bits(GOLDILOCKS, CENTRED, 2**62 - 1) == 63 and min_bits(GOLDILOCKS, CENTRED, 2**62) == 0
    assert min_bits(GOLDILOCKS, RESIDUE, 2**63 - 1) == 63 and min_bits(GOLDILOCKS, RESIDUE, 2**63) == 0
    assert min_bits(Q44, 2, 5) == 0
