"""GPU suite: the fixed-point operator norm and the operator-norm-bounded challenge sampler (ring_opnorm, ring_challenge and their
device forms on NttContext and CyclicNtt) against the Python-integer model (tests/ring_challenge_model.py).  Every comparison is
exact: both are integer functions of the stream.  The model reports the tries of every element, the norm of every candidate it
looked at and the draws that went past word 0; each case asserts that the model reaches the path the case exists for before it
compares — an unreached path is not claimed as tested.  The seeds and bounds were chosen with the model on the CPU."""
import numpy as np
import pytest

import prover_replay
import ring_challenge_model as model
import ring_sample_model
from ring_sample_model import GOLDILOCKS, Q14, Q44, Q60, key_from_seed

pytestmark = pytest.mark.gpu


def _keys(keys):
    return np.array(keys, dtype=np.uint64).reshape(-1, 4)


def _dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _context(pkg, q, n, cyclic):
    return pkg.CyclicNtt(n, modulus=q) if cyclic else pkg.NttContext(q, n, device=0)


# name -> (q, n, cyclic, count, kappa1, kappa2, T, max_tries, first seed, components, what the model must report)
#   "spread": tries hold a 1, a value >= 2 and a value >= 8;  "exhausted": every element is;  "mixed": accepted and exhausted elements;
#   "both": some candidate was rejected and some accepted;  "accepted": every first candidate passes
CASES = {
    "labrador": (Q14, 64, False, 48, 31, 10, 15, 64, 100, 16, "spread"),
    "labrador exhausted": (Q14, 64, False, 48, 31, 10, 11, 3, 100, 16, "exhausted"),
    "labrador mixed": (Q14, 64, False, 64, 31, 10, 14, 4, 100, 16, "mixed"),
    # sub-wave and odd sizes.  n = 2: every candidate of (1, 1) is +-1 +- 2X with norm sqrt(5), so both outcomes take two bounds
    "n2 rejects": (Q14, 2, False, 5, 1, 1, 2, 3, 1, 5, "exhausted"),
    "n2 accepts": (Q14, 2, False, 5, 1, 1, 3, 3, 1, 5, "accepted"),
    "n4": (Q14, 4, False, 24, 2, 1, 3, 2, 1, 24, "mixed"),
    "n4 ragged": (Q14, 4, False, 24, 1, 2, 4, 2, 1, 7, "both"),
    "n8": (Q14, 8, False, 24, 3, 2, 5, 3, 1, 24, "both"),
    "n16": (Q14, 16, False, 24, 5, 3, 6, 3, 1, 5, "both"),
    # cyclic: E holds e = 0 and e = n, where the sums are exact: a candidate with |sum c_i| = T sits on the bound and passes
    "cyclic n8": (GOLDILOCKS, 8, True, 24, 3, 2, 5, 2, 1, 24, "mixed"),
    "cyclic n64": (GOLDILOCKS, 64, True, 24, 31, 10, 15, 8, 1, 24, "both"),
    # large n: one wave per workgroup at n = 4096; 3000 steps are six chunks of first-attempt words
    "n256": (Q44, 256, False, 8, 31, 10, 18, 4, 1, 8, "both"),
    "n1024": (Q44, 1024, False, 8, 31, 10, 21, 4, 1, 8, "both"),
    "n4096": (Q44, 4096, False, 6, 31, 10, 23, 4, 1, 6, "both"),
    "n4096 dense": (Q44, 4096, False, 3, 2000, 1000, 205, 2, 1, 3, "both"),
    # extremes of the weights
    "all twos": (Q14, 64, False, 12, 0, 10, 12, 4, 1, 12, "both"),
    "full n64": (Q14, 64, False, 12, 40, 24, 21, 4, 1, 12, "both"),
    "full n16": (Q14, 16, False, 12, 10, 6, 9, 4, 1, 12, "both"),
}
_REFERENCES = {}


def _reference(oracle, name):
    """(want, tries, stats) of a case from the model, computed once, with the assertion that the model reaches the case's path."""
    if name not in _REFERENCES:
        q, n, cyclic, count, k1, k2, bound, max_tries, seed, components, path = CASES[name]
        keys = [key_from_seed(seed + g) for g in range(-(-count // components))]
        want, tries, stats = model.challenge(oracle, q, n, count, k1, k2, bound, max_tries, keys, components, cyclic=cyclic)
        t = tries.tolist()
        rejected = any(v == 0 or v > 1 for v in t)
        if path == "spread":
            assert 1 in t and any(v >= 2 for v in t) and any(v >= 8 for v in t) and 0 not in t, t
        elif path == "exhausted":
            assert t == [0] * count and not want.any(), t
        elif path == "mixed":
            assert 0 in t and any(v >= 1 for v in t), t
        elif path == "both":
            assert rejected and any(v >= 1 for v in t), t
        else:
            assert path == "accepted" and t == [1] * count, t
        _REFERENCES[name] = (want, tries, stats, keys)
    return _REFERENCES[name]


@pytest.mark.parametrize("name", list(CASES))
def test_challenges_and_tries_equal_the_model(pkg, oracle, name):
    import torch
    q, n, cyclic, count, k1, k2, bound, max_tries, _, components, _ = CASES[name]
    want, want_tries, stats, keys = _reference(oracle, name)
    if name == "labrador":
        assert sum(s.draws.past_word0 for s in stats) > 0, "a step of the shuffle must reach a later word of its attempt"
    if name == "n4096 dense":
        assert all(s.draws.past_word0 > 0 for s in stats)
    if name == "cyclic n8":
        assert any(norms[-1] == model.bound_of(bound) for norms in (s.norms for s in stats)), "a candidate must sit on the bound itself"
    ctx = _context(pkg, q, n, cyclic)
    got, tries = ctx.ring_challenge(count, k1, k2, bound, _keys(keys), components=components, max_tries=max_tries)
    assert tries.dtype == np.int32 and tries.tolist() == want_tries.tolist(), name
    assert np.array_equal(got, want), name
    for row, t in zip(got, tries):                               # the weights on the device output itself
        values, counts = np.unique(row, return_counts=True)
        have = dict(zip((int(v) for v in values), (int(c) for c in counts)))
        if t == 0:
            assert have == {0: n}
        else:
            assert have.get(1, 0) + have.get(q - 1, 0) == k1 and have.get(2, 0) + have.get(q - 2, 0) == k2 and have.get(0, 0) == n - k1 - k2
    # the device form on fresh buffers gives the host form
    d_keys = _dev(torch, _keys(keys))
    d_out, d_tries = torch.full((count, n), -1, dtype=torch.int64, device="cuda"), torch.full((count,), -1, dtype=torch.int32, device="cuda")
    ctx.ring_challenge_device(d_out.data_ptr(), d_tries.data_ptr(), count, k1, k2, bound, d_keys.data_ptr(), components, max_tries=max_tries,
                              stream=_stream(torch))
    torch.cuda.synchronize()
    assert np.array_equal(_host(d_out), want) and d_tries.cpu().tolist() == want_tries.tolist(), (name, "device form")
    ctx.close()


def test_accepted_challenges_are_below_the_bound_by_the_stand_alone_norm(pkg, oracle):
    q, n, cyclic, count, k1, k2, bound, max_tries, _, components, _ = CASES["labrador"]
    want, want_tries, stats, _ = _reference(oracle, "labrador")
    ctx = _context(pkg, q, n, cyclic)
    norms = ctx.ring_opnorm(want)
    assert norms.tolist() == [s.norms[-1] for s in stats]
    assert all(v <= model.bound_of(bound) for v in norms)
    assert all(x > model.bound_of(bound) for s in stats for x in s.norms[:-1])      # and every candidate before it was above
    ctx.close()


# ---- identity with LSR_RING_SAMPLE_BALL --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kappas", [(8, (1, 4, 8)), (64, (1, 32, 64)), (4096, (1, 2048, 3000, 4096))])
def test_without_twos_and_without_a_bound_it_is_ball_word_for_word(pkg, n, kappas):
    """kappa2 = 0, opnorm_bound = 0: the shared shuffle.  n = 4096, kappa = 3000 and 4096: past the 2048-word chunk of the BALL kernel
    and through six and eight of this one's 512-word chunks."""
    q, count, components = (Q14 if n <= 64 else Q44), 5, 2
    keys = _keys([key_from_seed(s) for s in (7, 8, 9)])
    ctx = pkg.NttContext(q, n, device=0)
    for kappa in kappas:
        ball = ctx.ring_sample(count, pkg.RING_SAMPLE_BALL, kappa, keys, components=components, domain=19, index_base=3)
        got, tries = ctx.ring_challenge(count, kappa, 0, 0, keys, components=components, max_tries=1, domain=19, index_base=3)
        assert np.array_equal(got, ball), (n, kappa)
        assert tries.tolist() == [1] * count
    ctx.close()


def test_without_a_bound_the_first_candidate_is_taken_whatever_its_norm(pkg, oracle):
    q, n, count = Q14, 64, 6
    keys = [key_from_seed(100)]
    want, want_tries, stats = model.challenge(oracle, q, n, count, 31, 10, 0, 64, keys, count)
    _, bounded, _ = model.challenge(oracle, q, n, count, 31, 10, 15, 64, keys, count)
    assert want_tries.tolist() == [1] * count and any(t > 1 for t in bounded.tolist())
    ctx = pkg.NttContext(q, n, device=0)
    got, tries = ctx.ring_challenge(count, 31, 10, 0, _keys(keys), max_tries=64)
    assert np.array_equal(got, want) and tries.tolist() == [1] * count
    ctx.close()


# ---- moduli ----------------------------------------------------------------------------------------------------------------------------------
def test_moduli_differ_only_in_the_stored_negatives(pkg, oracle):
    n, count, k1, k2, bound, max_tries = 64, 6, 31, 10, 15, 32
    keys = [key_from_seed(100)]
    centred = None
    for q, cyclic in [(Q14, False), (Q44, False), (Q60, False), (GOLDILOCKS, True)]:
        want, want_tries, stats = model.challenge(oracle, q, n, count, k1, k2, bound, max_tries, keys, count, cyclic=cyclic)
        assert any(t > 1 for t in want_tries.tolist()) and 0 not in want_tries.tolist()
        if not cyclic:                                           # one ring, one stream: the same integers under every modulus
            mine = [model.centred(row, q) for row in want]
            assert centred is None or mine == centred
            centred = mine
        ctx = _context(pkg, q, n, cyclic)
        got, tries = ctx.ring_challenge(count, k1, k2, bound, _keys(keys), max_tries=max_tries)
        assert np.array_equal(got, want) and tries.tolist() == want_tries.tolist(), q
        assert set(int(v) for v in np.unique(got)) <= {0, 1, 2, q - 1, q - 2}
        ctx.close()


# ---- keys ------------------------------------------------------------------------------------------------------------------------------------
def test_device_resident_digests_key_the_challenges(pkg, lib, oracle):
    """lsr_fs_challenge_batch_device -> ring_challenge_device with the digests as keys: count = 5 with components = 2 reads three
    digests, the last group ragged; index_base != 0."""
    import torch
    q, n, count, components, base, width = Q14, 64, 5, 2, 7, 24
    rng = np.random.default_rng(30)
    rows = rng.integers(0, q, size=(3, width), dtype=np.uint64)
    s = _stream(torch)
    d_rows = _dev(torch, rows)
    d_alpha = torch.zeros(3, dtype=torch.int64, device="cuda")
    d_hash = torch.zeros((3, 32), dtype=torch.uint8, device="cuda")
    d_out, d_tries = torch.zeros((count, n), dtype=torch.int64, device="cuda"), torch.zeros(count, dtype=torch.int32, device="cuda")
    assert lib.lsr_fs_challenge_batch_device(None, 0, d_rows.data_ptr(), width, 3, q, d_alpha.data_ptr(), d_hash.data_ptr(), s) == 0
    ctx = pkg.NttContext(q, n, device=0)
    ctx.ring_challenge_device(d_out.data_ptr(), d_tries.data_ptr(), count, 31, 10, 15, d_hash.data_ptr(), components, max_tries=32, index_base=base,
                              stream=s)
    torch.cuda.synchronize()
    digests = [prover_replay.challenge_derive([], rows[j], q)[1] for j in range(3)]
    assert [bytes(h) for h in d_hash.cpu().numpy()] == digests
    keys = [ring_sample_model.key_from_bytes(d) for d in digests]
    want, want_tries, _ = model.challenge(oracle, q, n, count, 31, 10, 15, 32, keys, components, index_base=base)
    shifted, _, _ = model.challenge(oracle, q, n, count, 31, 10, 15, 32, keys, components, index_base=0)
    assert not np.array_equal(want, shifted) and any(t > 1 for t in want_tries.tolist())
    assert np.array_equal(_host(d_out), want) and d_tries.cpu().tolist() == want_tries.tolist()
    got, tries = ctx.ring_challenge(count, 31, 10, 15, b"".join(digests), components=components, max_tries=32, index_base=base)
    assert np.array_equal(got, want) and tries.tolist() == want_tries.tolist()
    ctx.close()


# ---- the stand-alone norm ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cyclic", [(2, False), (8, False), (8, True), (64, False), (256, False), (4096, False), (4096, True)])
def test_norm_equals_the_model(pkg, n, cyclic):
    import torch
    q = GOLDILOCKS if cyclic else Q60
    rng = np.random.default_rng(n)
    top = model.MAX_COEFFICIENT
    rows = [rng.integers(-top, top + 1, size=n), rng.integers(-2, 3, size=n), np.full(n, top), np.array([top if i % 2 else -top for i in range(n)]),
            np.zeros(n, dtype=np.int64)]
    x = np.array([[int(v) % q for v in row] for row in rows], dtype=np.uint64)
    bad_word, bad_size, bad_negative = x[0].copy(), x[1].copy(), x[1].copy()
    bad_word[n - 1] = q
    bad_size[0] = top + 1
    bad_negative[n // 2] = q - top - 1
    x = np.concatenate([x, [bad_word, bad_size, bad_negative]])
    want = [model.opnorm(row, q, cyclic) for row in x]
    assert want[-3:] == [model.ALL_ONES] * 3 and model.ALL_ONES not in want[:-3] and want[4] == 0
    if cyclic:
        assert want[2] == (n * top) ** 2 << 60                   # all coefficients 2^15: the largest sums there are, at e = 0
    ctx = _context(pkg, q, n, cyclic)
    assert ctx.ring_opnorm(x).tolist() == want, (n, cyclic)
    assert ctx.ring_opnorm(x[0]) == want[0]
    d_x, d_out = _dev(torch, x), torch.zeros((len(x), 2), dtype=torch.int64, device="cuda")
    ctx.ring_opnorm_device(d_x.data_ptr(), len(x), d_out.data_ptr(), stream=_stream(torch))
    torch.cuda.synchronize()
    assert [int(lo) | (int(hi) << 64) for lo, hi in _host(d_out).tolist()] == want
    ctx.close()


# ---- graph capture ------------------------------------------------------------------------------------------------------------------------------
def test_device_forms_are_capturable_after_prepare(pkg, oracle):
    """ring_opnorm_prepare makes the table resident; behind it both device forms only enqueue.  One linear graph, replayed under changed
    keys."""
    import torch
    q, n, count, k1, k2, bound, max_tries = Q14, 64, 6, 31, 10, 15, 32
    ctx = pkg.NttContext(q, n, device=0)
    ctx.ring_opnorm_prepare()
    ctx.ring_opnorm_prepare()                                    # once is enough; twice is allowed
    key_sets = [_keys([key_from_seed(s)]) for s in (100, 101)]
    d_keys = _dev(torch, key_sets[0])
    d_out, d_norm = torch.zeros((count, n), dtype=torch.int64, device="cuda"), torch.zeros((count, 2), dtype=torch.int64, device="cuda")
    d_tries = torch.zeros(count, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        s = torch.cuda.current_stream().cuda_stream
        ctx.ring_challenge_device(d_out.data_ptr(), d_tries.data_ptr(), count, k1, k2, bound, d_keys.data_ptr(), count, max_tries=max_tries, stream=s)
        ctx.ring_opnorm_device(d_out.data_ptr(), count, d_norm.data_ptr(), stream=s)
    for keys in key_sets:
        d_keys.copy_(_dev(torch, keys))
        graph.replay()
        torch.cuda.synchronize()
        want, want_tries, stats = model.challenge(oracle, q, n, count, k1, k2, bound, max_tries, [[int(w) for w in keys[0]]], count)
        assert any(t > 1 for t in want_tries.tolist()) and 0 not in want_tries.tolist()
        assert np.array_equal(_host(d_out), want) and d_tries.cpu().tolist() == want_tries.tolist()
        assert [int(lo) | (int(hi) << 64) for lo, hi in _host(d_norm).tolist()] == [st.norms[-1] for st in stats]
    ctx.close()


# ---- a real context above the limit ----------------------------------------------------------------------------------------------------------
def test_contexts_above_4096_are_refused_by_every_call(pkg):
    ctx = pkg.NttContext(Q44, 8192, device=0)
    with pytest.raises(pkg.CoreError, match="lsr_ntt_ring_opnorm_prepare: .*LSR_RING_OPNORM_MAX_DEGREE = 4096"):
        ctx.ring_opnorm_prepare()
    with pytest.raises(pkg.CoreError, match="lsr_ntt_ring_opnorm_batch: .*LSR_RING_OPNORM_MAX_DEGREE = 4096"):
        ctx.ring_opnorm(np.zeros(8192, dtype=np.uint64))
    for bound in (0, 15):
        with pytest.raises(pkg.CoreError, match="lsr_ntt_ring_challenge_batch: .*LSR_RING_OPNORM_MAX_DEGREE = 4096"):
            ctx.ring_challenge(1, 31, 10, bound, pkg.ring_sample_key(1))
    ctx.close()
