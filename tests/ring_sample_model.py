"""Python-integer model of seeded ring sampling (batch.h "seeded ring sampling"): the streams, the one rejection
primitive draw(m; words; U) and the three kinds built on it.  TEST INFRASTRUCTURE.  The stream words come from the CPU oracle:
``stream_words`` for keys that are the expansion of a 64-bit seed, ``chacha20_block`` for full 256-bit keys.

Every sampling function also reports how far the draws went (``Stats``): a test that claims to cover the slow paths asserts that
those counts are non-zero for its case."""
import numpy as np

UNIFORM, BOUNDED, BALL = 0, 1, 2
MAX_WORDS = 64
TAG_WORD = 0x3152534C | (0x4D525453 << 32)      # "LSR1", "STRM"

Q14 = 12289
Q17 = 65537
Q_NORTH = 17592169062401
Q44 = 17592182243329
Q60 = 1152921504606584833
GOLDILOCKS = 2**64 - 2**32 + 1


def key_from_seed(seed):
    """{seed_lo, seed_hi, "LSR1", "STRM", 0, 0, 0, 0} as four little-endian 64-bit words."""
    return [int(seed) & (2**64 - 1), TAG_WORD, 0, 0]


def key_from_bytes(data):
    """32 bytes (a SHA3 digest) in their own order as four little-endian 64-bit words."""
    assert len(data) == 32
    return [int.from_bytes(data[8 * i:8 * i + 8], "little") for i in range(4)]


class Stream:
    """Word w of stream (key, domain, index): ChaCha20 block w // 8, 32-bit words 2 (w % 8) and 2 (w % 8) + 1; nonce {domain, index_lo,
    index_hi}."""

    def __init__(self, oracle, key, domain, index):
        self.oracle, self.key, self.domain, self.index = oracle, [int(k) for k in key], int(domain), int(index) & (2**64 - 1)
        self.seeded = self.key[1:] == [TAG_WORD, 0, 0]
        self.blocks = {}

    def words(self, first, count):
        if self.seeded:
            return self.oracle.stream_words(self.key[0], self.domain, self.index, first, count)
        return np.array([self.word(first + i) for i in range(count)], dtype=np.uint64)

    def word(self, w):
        assert 0 <= w < 1 << 28, "the block counter must not wrap"
        if self.seeded:
            return int(self.oracle.stream_words(self.key[0], self.domain, self.index, w, 1)[0])
        block = w // 8
        if block not in self.blocks:
            key32 = [(k >> s) & 0xFFFFFFFF for k in self.key for s in (0, 32)]
            out = self.oracle.chacha20_block(key32, block, [self.domain, self.index & 0xFFFFFFFF, self.index >> 32])
            self.blocks[block] = [int(out[2 * j]) | (int(out[2 * j + 1]) << 32) for j in range(8)]
        return self.blocks[block][w % 8]


class Stats:
    """Of the draws of one element: how many took a field other than field 0 of their first word (past_field0), how many took a
    later word (past_word0), and depth[a] = draws accepted from attempt word a."""

    def __init__(self):
        self.draws = self.past_field0 = self.past_word0 = self.consumed = 0
        self.depth = {}

    def note(self, attempt, field):
        self.draws += 1
        self.past_field0 += 1 if (attempt, field) != (0, 0) else 0
        self.past_word0 += 1 if attempt else 0
        self.depth[attempt] = self.depth.get(attempt, 0) + 1


def draw(m, word_at, bits, stats):
    """draw(m; word_at(0), word_at(1), ...; U = bits): the first L-bit field below m, fields in order within a word, words in order."""
    if m == 1:
        return 0                                         # consumes nothing
    width = (m - 1).bit_length()
    fields, mask = bits // width, (1 << width) - 1
    word = 0
    for attempt in range(MAX_WORDS):
        word = word_at(attempt)
        stats.consumed += 1
        for f in range(fields):
            c = (word >> (f * width)) & mask
            if c < m:
                stats.note(attempt, f)
                return c
    stats.note(MAX_WORDS, 0)
    return (word & mask) % m


def _element_uniform(stream, q, n, m, beta, stats):
    first = stream.words(0, n)
    width = (m - 1).bit_length()
    cand = first & np.uint64((1 << width) - 1)
    hit = cand < np.uint64(m)
    out = [0] * n
    for i in range(n):
        if hit[i]:                                       # field 0 of word i: what draw() returns first
            stats.note(0, 0)
            stats.consumed += 1
            r = int(cand[i])
        else:
            r = draw(m, lambda a, i=i: int(first[i]) if a == 0 else stream.word(a * n + i), 64, stats)
        v = r - beta
        out[i] = v if v >= 0 else q + v
    return out


def _element_ball(stream, q, n, kappa, stats):
    first = [int(w) for w in stream.words(0, kappa)]
    c = [0] * n
    for s in range(kappa):
        i = n - kappa + s
        j = draw(i + 1, lambda a, s=s: first[s] if a == 0 else stream.word(a * kappa + s), 63, stats)
        c[i] = c[j]
        c[j] = q - 1 if first[s] >> 63 else 1
    return c


def sample(oracle, q, n, count, kind, param, keys, components, domain=16, index_base=0):
    """-> ([count, n] uint64, [Stats per element]).  keys: a list of keys of four 64-bit words; element e uses keys[e // components] and
    stream index index_base + e % components."""
    assert components >= 1 and len(keys) >= -(-count // components)
    if kind == UNIFORM:
        assert param == 0
    elif kind == BOUNDED:
        assert 1 <= param <= (q - 1) // 2
    else:
        assert kind == BALL and 1 <= param <= n
    out, stats = np.zeros((count, n), dtype=np.uint64), []
    for e in range(count):
        stream = Stream(oracle, keys[e // components], domain, index_base + e % components)
        st = Stats()
        if kind == BALL:
            row = _element_ball(stream, q, n, param, st)
        else:
            row = _element_uniform(stream, q, n, q if kind == UNIFORM else 2 * param + 1, 0 if kind == UNIFORM else param, st)
        out[e] = np.array(row, dtype=np.uint64)
        stats.append(st)
    return out, stats


def first_rejection(oracle, seed, q, words, domain=16, index=0):
    """The first word of the stream's first `words` whose field 0 is not below q (UNIFORM at a modulus with one field per word), or None."""
    width = (q - 1).bit_length()
    assert 64 // width == 1
    w = oracle.stream_words(seed, domain, index, 0, words) & np.uint64((1 << width) - 1)
    bad = np.nonzero(w >= np.uint64(q))[0]
    return int(bad[0]) if bad.size else None
