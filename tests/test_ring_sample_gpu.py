"""GPU suite: seeded ring sampling on the device (ring_sample / ring_sample_device / ring_matrix_seeded on NttContext and CyclicNtt)
against the Python-integer model (tests/ring_sample_model.py).  Every comparison is exact: the samplers are integer functions of the
stream.  The model reports how many draws of a case went past field 0 and past word 0 of their stream; wherever a case exists to reach
a slow path of the kernels, the test asserts that count is non-zero before it compares — an unreached path is not claimed as tested."""
import numpy as np
import pytest

import prover_replay
import ring_sample_model as model
import ring_tile_model
from ring_sample_model import BALL, BOUNDED, GOLDILOCKS, Q14, Q17, Q44, Q60, Q_NORTH, UNIFORM

pytestmark = pytest.mark.gpu

KEY1 = model.key_from_seed(1)


def _keys(keys):
    return np.array(keys, dtype=np.uint64).reshape(-1, 4)


def _dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _centred_abs_max(x, q):
    v = x.astype(object)
    return int(np.where(v > q // 2, q - v, v).max())


# ---- 1. UNIFORM against the model ---------------------------------------------------------------------------------------------------
# (q, n, seed) -> what the model must report for element 0 (stream index 0): (draws past word 0, deepest attempt word)
UNIFORM_CASES = [(Q14, 2, 1), (Q14, 2, 178), (Q14, 4, 1), (Q14, 4, 67), (Q14, 8, 1), (Q14, 16, 1), (Q14, 256, 1), (Q14, 2048, 1), (Q17, 16, 1), (Q17, 4096, 1), (Q_NORTH, 4096, 135),
                 (Q44, 8192, 1), (Q60, 256, 1)]
SECOND_WORDS = {(Q14, 2048): 7, (Q14, 256): 1, (Q17, 4096): 454 + 56 + 8 + 3, (Q_NORTH, 4096): 1}


@pytest.mark.parametrize("q,n,seed", UNIFORM_CASES)
def test_uniform_equals_the_model(pkg, oracle, q, n, seed):
    count, key = 3, model.key_from_seed(seed)
    want, stats = model.sample(oracle, q, n, count, UNIFORM, 0, [key], count)
    if (q, n) in SECOND_WORDS:
        assert stats[0].past_word0 == SECOND_WORDS[(q, n)], "the case must reach the attempt loop"
    if n < 8 and seed != 1:                                    # one lane per element: these seeds reach a coefficient's second word
        assert stats[0].past_word0 == 1
    if q in (Q14, Q17):
        assert sum(s.past_field0 - s.past_word0 for s in stats) > 0, "the case must reach the later fields of a first word"
    if (q, n) == (Q17, 4096):
        assert max(stats[0].depth) == 4
    ctx = pkg.NttContext(q, n, device=0)
    assert ctx.uses_f64 == (q != Q60)
    got = ctx.ring_sample(count, pkg.RING_SAMPLE_UNIFORM, 0, pkg.ring_sample_key(seed))
    assert got.shape == (count, n) and int(got.max()) < q
    assert np.array_equal(got, want), (q, n)
    ctx.close()


def test_uniform_goldilocks_takes_the_whole_word(pkg, oracle):
    """L = 64: the mask is the full word and a rejection (probability 2^-32) is out of reach; every coefficient is its stream word."""
    n, count = 256, 3
    want, stats = model.sample(oracle, GOLDILOCKS, n, count, UNIFORM, 0, [KEY1], count)
    assert all(s.past_field0 == 0 for s in stats)
    assert np.array_equal(want[1], oracle.stream_words(1, 16, 1, 0, n))
    ntt = pkg.CyclicNtt(n)
    assert np.array_equal(ntt.ring_sample(count, pkg.RING_SAMPLE_UNIFORM, 0, _keys([KEY1])), want)
    ntt.close()


def test_large_cyclic_context_uniform_and_ball(pkg, oracle):
    """n = 2^18, above the two-pass sizes: the same UNIFORM kernel, and BALL with the polynomial in the output instead of LDS."""
    n = 1 << 18
    ntt = pkg.CyclicNtt(n)
    want, _ = model.sample(oracle, GOLDILOCKS, n, 1, UNIFORM, 0, [KEY1], 1, index_base=5)
    assert np.array_equal(ntt.ring_sample(1, pkg.RING_SAMPLE_UNIFORM, 0, _keys([KEY1]), index_base=5), want)
    for count, kappa in [(2, 60), (1, 40000)]:                  # 40000 steps: 20 chunks of first-attempt words, m down to 0.85 * 2^18
        want, stats = model.sample(oracle, GOLDILOCKS, n, count, BALL, kappa, [KEY1], count)
        if kappa == 40000:
            assert stats[0].past_field0 > 0 and stats[0].past_word0 > 0
        got = ntt.ring_sample(count, pkg.RING_SAMPLE_BALL, kappa, _keys([KEY1]))
        assert np.array_equal(got, want) and [int(np.count_nonzero(r)) for r in got] == [kappa] * count
    ntt.close()


# ---- 2. keys and indices ----------------------------------------------------------------------------------------------------------
def test_full_keys_ragged_groups_and_the_device_form(pkg, oracle):
    """Random 256-bit keys; count = 5 with components = 2: three keys, the last group ragged; the device form gives the host form."""
    import torch
    q, n, count, components = Q14, 256, 5, 2
    rng = np.random.default_rng(21)
    keys = rng.integers(0, 2**64, size=(3, 4), dtype=np.uint64)
    keys[0, 3] |= np.uint64(1 << 63)                           # the top bit of the key is used
    ctx = pkg.NttContext(q, n, device=0)
    for kind, param in [(UNIFORM, 0), (BOUNDED, 2), (BALL, 60)]:
        want, stats = model.sample(oracle, q, n, count, kind, param, [[int(w) for w in k] for k in keys], components, domain=3, index_base=9)
        got = ctx.ring_sample(count, kind, param, keys, components=components, domain=3, index_base=9)
        assert np.array_equal(got, want), kind
        d_keys, d_out = _dev(torch, keys), torch.zeros((count, n), dtype=torch.int64, device="cuda")
        ctx.ring_sample_device(d_out.data_ptr(), count, kind, param, d_keys.data_ptr(), components, domain=3, index_base=9, stream=_stream(torch))
        torch.cuda.synchronize()
        assert np.array_equal(_host(d_out), want), (kind, "device form")
    # one key given as its 32 bytes: the same words
    want, _ = model.sample(oracle, q, n, 2, UNIFORM, 0, [[int(w) for w in keys[0]]], 2, domain=3, index_base=9)
    assert np.array_equal(ctx.ring_sample(2, UNIFORM, 0, keys[0].tobytes(), domain=3, index_base=9), want)
    ctx.close()


@pytest.mark.parametrize("kind,param", [(UNIFORM, 0), (BALL, 3)])
def test_index_carries_into_the_high_nonce_word(pkg, oracle, kind, param):
    q, n, count, base = Q14, 16, 3, 2**32 - 1
    want, _ = model.sample(oracle, q, n, count, kind, param, [KEY1], count, index_base=base)
    low, _ = model.sample(oracle, q, n, 1, kind, param, [KEY1], 1, index_base=0)
    assert not np.array_equal(want[1], low[0]), "index 2^32 is not index 0"
    ctx = pkg.NttContext(q, n, device=0)
    assert np.array_equal(ctx.ring_sample(count, kind, param, _keys([KEY1]), index_base=base), want)
    ctx.close()


def test_device_form_is_capturable_from_the_first_call(pkg, oracle):
    """No workspace and no allocation: the very first call on a fresh context is the captured one.  Replayed twice under changed keys."""
    import torch
    q, n, count = Q17, 256, 4
    ctx = pkg.NttContext(q, n, device=0)
    key_sets = [_keys([model.key_from_seed(s) for s in pair]) for pair in ((1, 2), (3, 4))]
    d_keys = _dev(torch, key_sets[0])
    d_u, d_b = (torch.zeros((count, n), dtype=torch.int64, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        s = torch.cuda.current_stream().cuda_stream
        ctx.ring_sample_device(d_u.data_ptr(), count, UNIFORM, 0, d_keys.data_ptr(), 2, stream=s)
        ctx.ring_sample_device(d_b.data_ptr(), count, BALL, 60, d_keys.data_ptr(), 2, stream=s)
    for keys in key_sets:
        d_keys.copy_(_dev(torch, keys))
        graph.replay()
        torch.cuda.synchronize()
        listed = [[int(w) for w in k] for k in keys]
        want_u, stats = model.sample(oracle, q, n, count, UNIFORM, 0, listed, 2)
        assert sum(st.past_word0 for st in stats) > 0
        assert np.array_equal(_host(d_u), want_u) and np.array_equal(_host(d_u), ctx.ring_sample(count, UNIFORM, 0, keys, components=2))
        assert np.array_equal(_host(d_b), model.sample(oracle, q, n, count, BALL, 60, listed, 2)[0])
    ctx.close()


# ---- 3. BOUNDED ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q,n", [(Q14, 256), (Q_NORTH, 4096)])
def test_bounded_equals_the_model_and_is_short(pkg, oracle, q, n):
    ctx = pkg.NttContext(q, n, device=0)
    top = (q - 1) // 2
    for beta in (1, 2, 16384, 32767, top):
        if beta > top:                                         # q = 12289: 16384 and 32767 are refusals (test_refusals_that_read_the_context)
            continue
        want, stats = model.sample(oracle, q, n, 2, BOUNDED, beta, [KEY1], 2)
        if n == 4096 and beta == 16384:
            assert stats[0].past_word0 == 241                  # m = 32769: about half of the 16-bit fields are rejected, four to a word
        if beta == 1:
            assert stats[0].past_word0 == 0 and stats[0].past_field0 > 0
        got = ctx.ring_sample(2, pkg.RING_SAMPLE_BOUNDED, beta, _keys([KEY1]))
        assert np.array_equal(got, want), (q, n, beta)
        linf = ctx.ring_linf(got)
        assert int(linf.max()) <= beta and int(linf.max()) == _centred_abs_max(got, q)
        if beta <= 2:
            centred = np.where(got.astype(object) > q // 2, got.astype(object) - q, got.astype(object))
            assert centred.min() == -beta and centred.max() == beta
    uniform = ctx.ring_sample(2, pkg.RING_SAMPLE_UNIFORM, 0, _keys([KEY1]))
    shifted = (uniform.astype(object) + (q - top)) % q
    assert np.array_equal(ctx.ring_sample(2, pkg.RING_SAMPLE_BOUNDED, top, _keys([KEY1])), shifted.astype(np.uint64))
    ctx.close()


# ---- 4. BALL ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kappa", [(2, 1), (2, 2), (64, 39), (256, 60), (4096, 60), (4096, 4096)])
def test_ball_equals_the_model_with_exact_weight(pkg, oracle, n, kappa):
    import torch
    q = Q14 if n <= 256 else Q_NORTH
    want, stats = model.sample(oracle, q, n, 2, BALL, kappa, [KEY1], 2)
    if (n, kappa) == (4096, 4096):
        assert stats[0].past_word0 == 24                       # the only case whose steps reach a second word
    elif (n, kappa) == (4096, 60):
        assert stats[0].past_word0 == 0
    if (n, kappa) in ((64, 39), (4096, 4096)):
        assert stats[0].past_field0 > stats[0].past_word0
    ctx = pkg.NttContext(q, n, device=0)
    d_keys, d_out = _dev(torch, _keys([KEY1])), torch.zeros((2, n), dtype=torch.int64, device="cuda")
    ctx.ring_sample_device(d_out.data_ptr(), 2, pkg.RING_SAMPLE_BALL, kappa, d_keys.data_ptr(), 2, stream=_stream(torch))
    torch.cuda.synchronize()
    got = _host(d_out)
    for row in got:                                            # weight and +-1 on the device output itself
        assert int(np.count_nonzero(row)) == kappa and set(int(v) for v in np.unique(row)) <= {0, 1, q - 1}
    assert np.array_equal(got, want), (n, kappa)
    assert np.array_equal(ctx.ring_sample(2, pkg.RING_SAMPLE_BALL, kappa, _keys([KEY1])), want)
    ctx.close()


# ---- 5. the seeded matrix -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q,n", [(Q_NORTH, 4096), (Q14, 16), (Q44, 8192)])
def test_seeded_matrix_is_the_matrix_of_the_sampled_words(pkg, oracle, q, n):
    """n <= 4096: sampled and transformed in place (tile route); n = 8192: kept as sampled (composed route)."""
    rows, cols, base = 3, 5, 11
    rng = np.random.default_rng(n)
    ctx = pkg.NttContext(q, n, device=0)
    key = pkg.ring_sample_key(1)
    words = ctx.ring_sample(rows * cols, pkg.RING_SAMPLE_UNIFORM, 0, key, index_base=base)
    assert np.array_equal(words[7], model.sample(oracle, q, n, 1, UNIFORM, 0, [KEY1], 1, index_base=base + 7)[0][0]), "entry [1][2]"
    x = rng.integers(0, q, size=(2, cols, n), dtype=np.uint64)
    seeded, plain = ctx.ring_matrix_seeded(key, rows, cols, index_base=base), ctx.ring_matrix(words.reshape(rows, cols, n))
    assert (seeded.rows, seeded.cols, seeded.row_block) == (rows, cols, plain.row_block)
    y = seeded.matvec(x)
    assert np.array_equal(y, plain.matvec(x)), (q, n)
    if n == 16:
        assert np.array_equal(y, np.array(ring_tile_model.schoolbook_matvec(words.reshape(rows, cols, n), x, q, -1), dtype=np.uint64))
    seeded.close()
    plain.close()
    ctx.close()


def test_seeded_matrix_refusals_that_read_the_context(pkg, lib):
    key = pkg.ring_sample_key(1)
    large = pkg.CyclicNtt(1 << 18)
    with pytest.raises(pkg.CoreError, match="131072"):
        large.ring_matrix_seeded(key, 1, 1)
    large.close()
    n = 4096
    ctx = pkg.NttContext(Q_NORTH, n, device=0)
    rows, cols = 129, pkg.RING_MATVEC_MAX_MATRIX_BYTES // (n * 8) // 128
    assert rows * cols * 16 <= pkg.RING_MATVEC_MAX_MATRIX_BYTES < rows * cols * n * 8
    for index_base in (0, 2**64 - 1):                           # the byte cap comes before the index overflow
        with pytest.raises(pkg.CoreError, match="LSR_RING_MATVEC_MAX_MATRIX_BYTES"):
            ctx.ring_matrix_seeded(key, rows, cols, index_base=index_base)
    with pytest.raises(pkg.CoreError, match="lsr_ntt_ring_matrix_create_seeded: .*overflows"):
        ctx.ring_matrix_seeded(key, 3, 5, index_base=2**64 - 15)
    mat = ctx.ring_matrix_seeded(key, 3, 5, index_base=2**64 - 16)      # the last index is 2^64 - 2
    mat.close()
    ctx.close()


# ---- 6. rows -> transcript -> challenge -> fold without leaving the device --------------------------------------------------------------
def test_chain_from_rows_to_folded_rows_stays_on_the_device(pkg, lib, oracle):
    """commit_rows_device -> lsr_fs_challenge_batch_device (digests) -> ring_sample_device(BALL, keys = the digests) ->
    ring_combine_rows_device.  Challenge polynomial (j, i) is the BALL element of stream index i under the digest of row j; its -1 is
    t - 1, the plaintext modulus the fold centres by, so the sampling context is the ring of the plaintext modulus."""
    import torch
    outputs, terms, kappa = 2, 2, 60
    lwe = pkg.LweContext(pkg.Params(), key_seed=0xFEED)
    n, t, q, W = lwe.ring_degree, lwe.plain_modulus, lwe.commit_modulus, lwe.commitment_words
    assert (n, lwe.module_rank) == (4096, 2) and outputs * terms * kappa <= lwe.combine_max_weight
    ring = pkg.NttContext(t, n, device=0)
    rng = np.random.default_rng(5)
    msgs = rng.integers(0, 2**20, size=(terms, 7), dtype=np.uint64)
    keys = lwe.commit_keys(msgs, rng.integers(1, 2**62, size=terms, dtype=np.uint64))
    s = _stream(torch)
    d_msgs, d_keys = _dev(torch, msgs), _dev(torch, keys)
    d_rows = torch.zeros((terms, W), dtype=torch.int64, device="cuda")
    d_alpha = torch.zeros(terms, dtype=torch.int64, device="cuda")
    d_hash = torch.zeros((terms, 32), dtype=torch.uint8, device="cuda")
    d_polys = torch.zeros((outputs, terms, n), dtype=torch.int64, device="cuda")
    d_out = torch.zeros((outputs, W), dtype=torch.int64, device="cuda")
    d_status = torch.zeros(outputs, dtype=torch.int32, device="cuda")
    lwe.commit_rows_device(d_msgs.data_ptr(), 7, terms, d_keys.data_ptr(), d_rows.data_ptr(), s)
    assert lib.lsr_fs_challenge_batch_device(None, 0, d_rows.data_ptr(), W, terms, q, d_alpha.data_ptr(), d_hash.data_ptr(), s) == 0
    ring.ring_sample_device(d_polys.data_ptr(), outputs * terms, pkg.RING_SAMPLE_BALL, kappa, d_hash.data_ptr(), terms, stream=s)
    lwe.ring_combine_rows_device(d_rows.data_ptr(), terms, d_polys.data_ptr(), outputs, d_out.data_ptr(), d_status.data_ptr(), term_stride=0, stream=s)
    torch.cuda.synchronize()
    assert d_status.cpu().tolist() == [1] * outputs
    rows = _host(d_rows)
    digests = [prover_replay.challenge_derive([], rows[j], q)[1] for j in range(outputs)]
    assert [bytes(h) for h in d_hash.cpu().numpy()] == digests
    polys, _ = model.sample(oracle, t, n, outputs * terms, BALL, kappa, [model.key_from_bytes(d) for d in digests], terms)
    assert np.array_equal(_host(d_polys).reshape(-1, n), polys)
    want_rows, want_status = lwe.ring_combine_rows(rows, polys.reshape(outputs, terms, n), term_stride=0)
    assert want_status.tolist() == [1] * outputs and np.array_equal(_host(d_out), want_rows)
    ring.close()
    lwe.close()


# ---- 7. refusals that read the context ------------------------------------------------------------------------------------------------
def test_refusals_that_read_the_context(pkg, lib):
    """UNIFORM with a param, BOUNDED outside [1, (q - 1) / 2], BALL outside [1, n] — each also with count == 0 and with an index that
    overflows, which are looked at later; then the empty call (0); then the index overflow."""
    import torch
    q, n = Q14, 256
    ctx = pkg.NttContext(q, n, device=0)
    d, d_keys = torch.zeros((2, n), dtype=torch.int64, device="cuda"), _dev(torch, _keys([KEY1]))
    p, s = d.data_ptr(), _stream(torch)
    host_out, host_keys = np.zeros((2, n), dtype=np.uint64), _keys([KEY1])

    def call(device, count, kind, param, components=1, index_base=0):
        if device:
            return lib.lsr_ntt_ring_sample_batch_device(ctx.handle, p, count, kind, param, d_keys.data_ptr(), components, 16, index_base, s)
        return lib.lsr_ntt_ring_sample_batch(ctx.handle, host_out.ctypes.data, count, kind, param, host_keys.ctypes.data, components, 16, index_base)
    for device in (False, True):
        name = "lsr_ntt_ring_sample_batch_device" if device else "lsr_ntt_ring_sample_batch"
        bad = [(UNIFORM, 1, "UNIFORM"), (UNIFORM, 2**64 - 1, "UNIFORM"), (BOUNDED, 0, "BOUNDED"), (BOUNDED, (q - 1) // 2 + 1, "BOUNDED"),
               (BOUNDED, 16384, "BOUNDED"), (BOUNDED, 32767, "BOUNDED"), (BOUNDED, 2**63, "BOUNDED"), (BALL, 0, "BALL"), (BALL, n + 1, "BALL"),
               (BALL, 2**32 + 1, "BALL")]
        for kind, param, named in bad:
            for count, index_base in [(1, 0), (0, 0), (1, 2**64 - 1), (0, 2**64 - 1)]:
                assert call(device, count, kind, param, index_base=index_base) == -1, (kind, param)
                msg = pkg._abi.last_error()
                assert msg.startswith(name + ":") and named in msg and "overflow" not in msg, msg
        for kind, param in [(UNIFORM, 0), (BOUNDED, (q - 1) // 2), (BALL, n)]:
            assert call(device, 0, kind, param, index_base=2**64 - 1) == 0          # the empty call comes before the index overflow
            assert call(device, 1, kind, param, index_base=2**64 - 1) == -1 and "overflows" in pkg._abi.last_error()
            assert call(device, 1, kind, param, components=2**64 - 1, index_base=1) == -1 and "overflows" in pkg._abi.last_error()
            assert call(device, 1, kind, param, components=2**64 - 2, index_base=1) == 0
    torch.cuda.synchronize()
    ctx.close()
