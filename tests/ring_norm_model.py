"""Python-integer model of the norms and projections of ring vectors (batch.h "norms and projections of ring vectors"):
the exact l2 norm squared, the Johnson-Lindenstrauss projection and the rows of its matrix.  TEST INFRASTRUCTURE.  The stream words
come from ``ring_sample_model.Stream``, that is from the CPU oracle's ``stream_words`` / ``chacha20_block``.

``project`` sums in numpy's wrapping int64, which is exact whenever the true sum fits 64 bits — the contract's len * bound <= 2^63 - 1;
``project_ints`` is the same sum in Python integers, and the model's own tests hold the two against each other at the bound."""
import numpy as np

from ring_sample_model import Stream, key_from_bytes, key_from_seed  # noqa: F401  (re-exported for the tests)

ROWS = 256
SATURATED = 2**128 - 1


def centred(v, q):
    return v if v <= q // 2 else v - q


def entry(word, e):
    """pi at position 32 w + e from stream word w: f = (word >> 2 e) & 3 -> (f & 1) - (f >> 1), i.e. 0, +1, -1, 0."""
    f = (int(word) >> (2 * e)) & 3
    return (f & 1) - (f >> 1)


def row_signs(stream, length):
    """pi[r][0 .. length) of the row whose stream is given, as int8."""
    words = np.asarray(stream.words(0, -(-length // 32)), dtype=np.uint64)
    f = ((words[:, None] >> (np.arange(32, dtype=np.uint64) * np.uint64(2))[None, :]) & np.uint64(3)).reshape(-1)[:length].astype(np.int8)
    return (f & 1) - (f >> 1)


def matrix_signs(oracle, length, key, domain=17, index_base=0, rows_first=0, rows=ROWS):
    """[rows, length] int8: rows rows_first .. of the matrix of (key, index_base)."""
    return np.stack([row_signs(Stream(oracle, key, domain, index_base + rows_first + r), length) for r in range(rows)])


def project_matrix(oracle, q, n, width, key, rows_first=0, rows=ROWS, domain=17, index_base=0):
    """[rows, width, n] uint64 with words 0, 1, q - 1."""
    signs = matrix_signs(oracle, width * n, key, domain, index_base, rows_first, rows).astype(object)
    return np.where(signs < 0, q - 1, signs).astype(np.uint64).reshape(rows, width, n)


def status_of(words, q, bound):
    """1 done, -1 a word >= q, 0 some |centred| above bound (no word >= q)."""
    if any(v >= q for v in words):
        return -1
    return 0 if any(abs(centred(v, q)) > bound for v in words) else 1


def project(oracle, q, x, bound, keys, components, domain=17, index_base=0):
    """x [count, width, n] -> (int64 [count, 256], int32 [count]).  Vector j uses keys[j // components] and the streams
    index_base + 256 (j % components) + r."""
    x = np.asarray(x, dtype=np.uint64)
    count, length = x.shape[0], x.shape[1] * x.shape[2]
    assert 1 <= bound <= q // 2 and length * bound <= 2**63 - 1 and length <= 2**32
    assert components >= 1 and len(keys) >= -(-count // components)
    out, status, cache = np.zeros((count, ROWS), dtype=np.int64), np.zeros(count, dtype=np.int32), {}
    for j in range(count):
        words = x[j].reshape(-1)
        status[j] = status_of(words.tolist(), q, bound)
        if status[j] != 1:
            continue
        c = np.where(words > np.uint64(q // 2), words - np.uint64(q), words).view(np.int64)      # v - q wraps to the negative word
        who = (tuple(int(k) for k in keys[j // components]), j % components)
        if who not in cache:
            cache[who] = matrix_signs(oracle, length, keys[j // components], domain, index_base + ROWS * (j % components))
        signs = cache[who]
        out[j] = np.concatenate([signs[r:r + 32].astype(np.int64) @ c for r in range(0, ROWS, 32)])      # (integer matmul wraps)
    return out, status


def project_ints(oracle, q, words, key, domain=17, index=0):
    """The 256 sums of one vector (flattened canonical words) in Python integers; row r is the stream (key, domain, index + r)."""
    c = [centred(int(v), q) for v in words]
    out = []
    for r in range(ROWS):
        stream = Stream(oracle, key, domain, index + r)
        out.append(sum(entry(stream.word(pos // 32), pos % 32) * c[pos] for pos in range(len(c))))
    return out


def l2sq(q, x):
    """x [count, width, n] -> [count] Python ints: sum of centred^2, or 2^128 - 1 (a word >= q, or a sum that does not fit below it)."""
    out = []
    for vec in np.asarray(x, dtype=np.uint64).reshape(len(x), -1).tolist():
        total = sum(centred(v, q) ** 2 for v in vec)
        out.append(SATURATED if any(v >= q for v in vec) or total >= SATURATED else total)
    return out


# ---- the model's own tests (collected by tests/test_ring_norm_abi.py) ------------------------------------------------------------------
def test_entry_map_by_hand():
    word = 0b11_10_01_00 | (0b01 << 62) | (0b10 << 32)      # fields 0 .. 3 = 0, 1, 2, 3; field 16 = 2; field 31 = 1
    assert [entry(word, e) for e in range(4)] == [0, 1, -1, 0]
    assert entry(word, 16) == -1 and entry(word, 31) == 1 and entry(word, 15) == 0 and entry(word, 30) == 0

    class OneWord:
        def words(self, first, count):
            assert (first, count) == (0, 1)
            return np.array([word], dtype=np.uint64)
    signs = row_signs(OneWord(), 32).tolist()
    assert signs == [entry(word, e) for e in range(32)] and sum(abs(s) for s in signs) == 4
    assert row_signs(OneWord(), 3).tolist() == [0, 1, -1]      # a vector that ends inside the word


def test_project_is_the_sum_over_its_own_matrix_rows(oracle):
    q, n, width, count = 12289, 8, 5, 5                          # len 40: crosses a word and ends inside one
    rng = np.random.default_rng(40)
    x = rng.integers(0, q, size=(count, width, n), dtype=np.uint64)
    keys = [key_from_seed(3), key_from_bytes(bytes(range(32))), key_from_seed(4)]
    out, status = project(oracle, q, x, q // 2, keys, 2, 17, 9)      # components 2: a ragged last group
    assert status.tolist() == [1] * count
    for j in range(count):
        rows = project_matrix(oracle, q, n, width, keys[j // 2], 0, ROWS, 17, 9 + ROWS * (j % 2))
        signs = [[centred(v, q) for v in row] for row in rows.reshape(ROWS, -1).tolist()]
        assert set(v for row in signs for v in row) <= {-1, 0, 1}
        c = [centred(v, q) for v in x[j].reshape(-1).tolist()]
        assert out[j].tolist() == [sum(s * v for s, v in zip(row, c)) for row in signs], j
        assert out[j].tolist() == project_ints(oracle, q, x[j].reshape(-1).tolist(), keys[j // 2], 17, 9 + ROWS * (j % 2)), j
    assert np.array_equal(project_matrix(oracle, q, n, width, keys[0], 7, 3, 17, 9), project_matrix(oracle, q, n, width, keys[0], 0, ROWS, 17, 9)[7:10])


def test_wrapping_sum_is_exact_at_the_accumulator_bound(oracle):
    q, n = 1152921504606584833, 8                                # len * floor(q/2) = 2^62 - ...: inside int64, far outside float64
    for v in (q // 2, q - q // 2):                               # +floor(q/2) and -floor(q/2)
        x = np.full((1, 1, n), v, dtype=np.uint64)
        out, status = project(oracle, q, x, q // 2, [key_from_seed(60)], 1)
        assert status.tolist() == [1]
        assert out[0].tolist() == project_ints(oracle, q, x.reshape(-1).tolist(), key_from_seed(60))
        assert max(abs(p) for p in out[0].tolist()) > 2**60      # the case does reach the top of the range


def test_status_and_saturation_rules():
    q = 12289
    assert status_of([0, q - 1, q // 2], q, q // 2) == 1
    assert status_of([5, q - 6], q, 5) == 0 and status_of([5, q - 5], q, 5) == 1
    assert status_of([q, 6], q, 5) == -1                         # a word >= q outranks the bound
    assert l2sq(q, [[[1, q - 2], [q // 2, q // 2 + 1]]]) == [1 + 4 + 2 * (q // 2) ** 2]
    assert l2sq(q, [[[q, 0]], [[3, 0]]]) == [SATURATED, 9]
    gold = 2**64 - 2**32 + 1
    assert l2sq(gold, [[[gold // 2] * 4]]) == [4 * (gold // 2) ** 2] and 4 * (gold // 2) ** 2 < SATURATED
    assert l2sq(gold, [[[gold // 2] * 8]]) == [SATURATED]


JL_CASES = [(12289, 256, 3, 11), (17592169062401, 4096, 2, 12), (1152921504606584833, 8, 5, 13)]


def test_projection_preserves_the_norm_for_the_fixed_seeds(oracle):
    """sum_r p_r^2 has mean 128 |s|^2 and a relative deviation of about sqrt(2 / 256) = 0.09: [1/2, 3/2] is over 5 sigma wide."""
    for q, n, width, seed in JL_CASES:
        rng = np.random.default_rng(seed)
        bound = min(q // 2, 1 << 20)
        x = (rng.integers(-bound, bound + 1, size=(1, width, n)) % q).astype(np.uint64)
        out, status = project(oracle, q, x, bound, [key_from_seed(seed)], 1)
        assert status.tolist() == [1]
        got, norm = sum(p * p for p in out[0].tolist()), l2sq(q, x)[0]
        assert 64 * norm <= got <= 192 * norm, (q, n, width, got / (128 * norm))
