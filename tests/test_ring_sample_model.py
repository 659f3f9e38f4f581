"""CPU suite: the Python-integer model of seeded ring sampling (tests/ring_sample_model.py) has the properties the contract states, and
the facts the GPU tests rely on to reach the slow paths hold for it: which seeds, moduli and sizes meet a rejected field or word.
Those facts are re-derived here from the model and the CPU oracle's ChaCha20 stream; nothing is taken from a document."""
import hashlib

import numpy as np
import pytest

import ring_sample_model as model
from ring_sample_model import BALL, BOUNDED, Q14, Q17, Q_NORTH, UNIFORM

KEY1 = model.key_from_seed(1)


def _centred(x, q):
    v = x.astype(object)
    return np.where(v > q // 2, v - q, v)


def test_m_equal_one_consumes_nothing():
    stats = model.Stats()

    def never(_):
        raise AssertionError("draw(1) read a word")
    assert model.draw(1, never, 63, stats) == 0 and stats.consumed == 0 and stats.draws == 0


def test_draw_scans_fields_then_words_and_is_total():
    stats = model.Stats()
    # m = 5: L = 3, U = 64 -> 21 fields, U = 63 -> 21 fields; m = 2^63 + 1: L = 64 -> one field of the whole word (no shift by 64)
    assert model.draw(5, lambda a: 0b100_111_110, 64, stats) == 4 and stats.past_field0 == 1 and stats.past_word0 == 0
    all_bad = (1 << 63) - 1                                    # 21 fields of 7
    assert model.draw(5, lambda a: all_bad if a == 0 else 3, 63, stats) == 3 and stats.past_word0 == 1
    assert model.draw(2**63 + 1, lambda a: 2**64 - 1 if a < 2 else 2**63, 64, stats) == 2**63 and stats.depth[2] == 1
    # bit 63 is no candidate at U = 63: m = 2^62 + 1 -> L = 63, one field of the low 63 bits
    assert model.draw(2**62 + 1, lambda a: (1 << 63) | 5, 63, stats) == 5
    # never accepted: field 0 of the last word mod m, after exactly 64 words
    seen = []
    assert model.draw(5, lambda a: seen.append(a) or all_bad - a % 2, 64, stats) == ((all_bad - 1) & 7) % 5 and seen == list(range(64))


def test_key_from_bytes_is_the_digest_in_its_own_byte_order():
    digest = hashlib.sha3_256(b"ring").digest()
    assert b"".join(int(w).to_bytes(8, "little") for w in model.key_from_bytes(digest)) == digest


def test_full_keys_and_seed_keys_share_one_stream_definition(oracle):
    """A seed key read through chacha20_block (as a full key would be) gives the words stream_words gives."""
    by_seed = model.Stream(oracle, model.key_from_seed(77), 16, 2**32 - 1)
    as_full = model.Stream(oracle, model.key_from_seed(77), 16, 2**32 - 1)
    as_full.seeded = False
    assert by_seed.seeded and [int(w) for w in by_seed.words(5, 20)] == [as_full.word(5 + i) for i in range(20)]


@pytest.mark.parametrize("n,kappa", [(2, 1), (2, 2), (64, 39), (256, 60), (4096, 60)])
def test_ball_weight_is_exactly_kappa(oracle, n, kappa):
    out, _ = model.sample(oracle, Q14 if n <= 2048 else Q_NORTH, n, 2, BALL, kappa, [KEY1], 2)
    q = Q14 if n <= 2048 else Q_NORTH
    for row in out:
        assert set(int(v) for v in row) <= {0, 1, q - 1} and int(np.count_nonzero(row)) == kappa


@pytest.mark.parametrize("beta", [1, 2])
def test_bounded_stays_inside_and_attains_both_ends(oracle, beta):
    out, _ = model.sample(oracle, Q14, 256, 1, BOUNDED, beta, [KEY1], 1)
    c = _centred(out[0], Q14)
    assert c.min() == -beta and c.max() == beta


def test_bounded_at_the_largest_beta_is_the_shifted_uniform(oracle):
    beta = (Q14 - 1) // 2
    u, _ = model.sample(oracle, Q14, 16, 2, UNIFORM, 0, [KEY1], 2)
    b, _ = model.sample(oracle, Q14, 16, 2, BOUNDED, beta, [KEY1], 2)
    assert np.array_equal(b, (u + np.uint64(Q14 - beta)) % np.uint64(Q14))


def test_components_pick_keys_and_indices(oracle):
    keys = [model.key_from_seed(s) for s in (3, 4, 5)]
    out, _ = model.sample(oracle, Q14, 16, 5, UNIFORM, 0, keys, 2, index_base=7)
    for e, (k, idx) in enumerate([(0, 7), (0, 8), (1, 7), (1, 8), (2, 7)]):
        one, _ = model.sample(oracle, Q14, 16, 1, UNIFORM, 0, [keys[k]], 1, index_base=idx)
        assert np.array_equal(out[e], one[0]), e


# ---- the facts the GPU cases lean on: seed 1, domain 16, index 0 ---------------------------------------------------------------
def test_uniform_q65537_goes_five_words_deep(oracle):
    _, stats = model.sample(oracle, Q17, 4096, 1, UNIFORM, 0, [KEY1], 1)
    assert stats[0].depth == {0: 3575, 1: 454, 2: 56, 3: 8, 4: 3}


def test_uniform_q12289_reaches_a_second_word(oracle):
    for n, want in [(2048, 7), (256, 1)]:
        _, stats = model.sample(oracle, Q14, n, 1, UNIFORM, 0, [KEY1], 1)
        assert stats[0].past_word0 == want and stats[0].past_field0 > want, n


def test_uniform_q_north_first_rejection_is_seed_135(oracle):
    for seed in range(1, 135):
        assert model.first_rejection(oracle, seed, Q_NORTH, 8192) is None, seed
    assert model.first_rejection(oracle, 135, Q_NORTH, 8192) == 1756
    _, stats = model.sample(oracle, Q_NORTH, 4096, 1, UNIFORM, 0, [model.key_from_seed(135)], 1)
    assert stats[0].depth == {0: 4095, 1: 1}                   # coefficient 1756 takes word 4096 + 1756 = 5852


def test_bounded_q_north_second_words(oracle):
    _, half = model.sample(oracle, Q_NORTH, 4096, 1, BOUNDED, 16384, [KEY1], 1)
    assert half[0].past_word0 == 241
    _, one = model.sample(oracle, Q_NORTH, 4096, 1, BOUNDED, 1, [KEY1], 1)
    assert one[0].past_word0 == 0 and one[0].past_field0 > 0   # m = 3: a quarter of the 2-bit fields is rejected, 32 fields a word


def test_ball_second_words_only_at_full_weight(oracle):
    _, full = model.sample(oracle, Q_NORTH, 4096, 1, BALL, 4096, [KEY1], 1)
    assert full[0].past_word0 == 24
    _, sparse = model.sample(oracle, Q_NORTH, 4096, 1, BALL, 60, [KEY1], 1)
    assert sparse[0].past_word0 == 0
    _, mid = model.sample(oracle, Q14, 64, 1, BALL, 39, [KEY1], 1)
    assert mid[0].past_field0 > 0 and mid[0].past_word0 == 0      # m = 26 .. 64 in 5- and 6-bit fields


def test_small_degrees_reach_a_second_word_at_these_seeds(oracle):
    """n = 2 and n = 4 run one lane per element on the device; seeds 178 and 67 are the first whose element 0 rejects a whole word."""
    for n, seed in [(2, 178), (4, 67)]:
        _, stats = model.sample(oracle, Q14, n, 1, UNIFORM, 0, [model.key_from_seed(seed)], 1)
        assert stats[0].depth == {0: n - 1, 1: 1}, n
        for earlier in range(1, seed):
            _, none = model.sample(oracle, Q14, n, 1, UNIFORM, 0, [model.key_from_seed(earlier)], 1)
            assert none[0].past_word0 == 0, (n, earlier)
