"""GPU suite: bit-packed ring elements (ring_pack, ring_unpack and their device forms on NttContext and CyclicNtt) against the
Python-integer model (tests/ring_pack_model.py).  Every comparison is exact, word for word and status for status, in the host form
and in the device form.  Shapes are the smallest at which each mechanism can fail: n = 2 and 16 (one lane per element, padding),
n = 64 (one group per element, several elements per workgroup), n = 128, n = 4096 (an element spans workgroups: the status goes
through atomicMin) and n = 2^16 with the only bad coefficient in the last 64 of element 0."""
import numpy as np
import pytest

import prover_replay
import ring_pack_model as model
from ring_pack_model import CENTRED, RESIDUE
from ring_sample_model import GOLDILOCKS, Q14, Q44, Q60

pytestmark = pytest.mark.gpu

ALL_BITS = [1, 2, 3, 11, 13, 32, 33, 44, 45, 63]


def _dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _context(pkg, q, n):
    return pkg.CyclicNtt(n, modulus=q) if q == GOLDILOCKS else pkg.NttContext(q, n, device=0)


def _elements(rng, q, n, count, bits, mode):
    """count elements: in range with the end values first and last (status 1); one beyond each end (status 0); a word >= q together
    with an out-of-range one (status -1); then in-range ones again — a bad element between good ones.  Where the modulus does not
    reach the end of the field's range, the elements beyond the range do not exist and in-range ones take their place."""
    lo, hi = model.field_range(mode, bits)
    half = (q - 1) // 2
    x = [model.in_range_element(rng, n, q, bits, mode) for _ in range(count)]
    beyond = [hi + 1] if mode == RESIDUE else [hi + 1, lo - 1]
    for k, v in enumerate(beyond):
        if 1 + k < count and (abs(v) <= half if mode == CENTRED else v < q):
            x[1 + k][(n // 2 + k) % n] = v % q
    if count > 3:
        x[3][n - 1] = q if q == GOLDILOCKS else q + 5
        if (hi + 1 <= half if mode == CENTRED else hi + 1 < q):
            x[3][0] = hi + 1
    return np.array(x, dtype=np.uint64)


def _both_forms(torch, ctx, x, bits, mode, offset=0):
    """(words, status) of the host form, asserted equal to the device form; offset: the device buffers start that many words into
    their allocations (1: 8-byte but not 16-byte aligned)"""
    count, n = x.shape
    wpe = model.words(n, bits)
    words, status = ctx.ring_pack(x, bits, mode)
    d_x = torch.zeros(count * n + offset, dtype=torch.int64, device="cuda")
    d_x[offset:].copy_(_dev(torch, x).reshape(-1))
    d_w = torch.full((count * wpe + offset,), -1, dtype=torch.int64, device="cuda")
    d_s = torch.full((count,), 7, dtype=torch.int32, device="cuda")
    ctx.ring_pack_device(d_w.data_ptr() + 8 * offset, d_s.data_ptr(), d_x.data_ptr() + 8 * offset, count, bits, mode, stream=_stream(torch))
    torch.cuda.synchronize()
    assert np.array_equal(_host(d_w)[offset:].reshape(count, wpe), words) and d_s.cpu().tolist() == status.tolist()
    assert (_host(d_w)[:offset] == 2**64 - 1).all()
    return words, status


def _unpack_both_forms(torch, ctx, words, n, bits, mode, offset=0):
    count, wpe = words.shape
    x, status = ctx.ring_unpack(words, bits, mode)
    d_w = torch.zeros(count * wpe + offset, dtype=torch.int64, device="cuda")
    d_w[offset:].copy_(_dev(torch, words).reshape(-1))
    d_x = torch.full((count * n + offset,), -1, dtype=torch.int64, device="cuda")
    d_s = torch.full((count,), 7, dtype=torch.int32, device="cuda")
    ctx.ring_unpack_device(d_x.data_ptr() + 8 * offset, d_s.data_ptr(), d_w.data_ptr() + 8 * offset, count, bits, mode, stream=_stream(torch))
    torch.cuda.synchronize()
    assert np.array_equal(_host(d_x)[offset:].reshape(count, n), x) and d_s.cpu().tolist() == status.tolist()
    assert (_host(d_x)[:offset] == 2**64 - 1).all()
    return x, status


# (q, n, count): every context kind, every kernel path; counts that are no multiple of the elements per workgroup (8 at n = 64)
SHAPES = [(Q44, 2, 301), (Q44, 16, 67), (Q44, 64, 13), (Q44, 128, 7), (Q44, 4096, 5), (Q60, 64, 5), (Q60, 1024, 3), (GOLDILOCKS, 16, 5),
          (GOLDILOCKS, 64, 9), (GOLDILOCKS, 512, 3), (Q14, 64, 11), (Q14, 2, 5), (Q14, 1024, 4)]


@pytest.mark.parametrize("mode", [CENTRED, RESIDUE])
@pytest.mark.parametrize("q,n,count", SHAPES)
def test_pack_and_unpack_equal_the_model(pkg, q, n, count, mode):
    import torch
    ctx = _context(pkg, q, n)
    rng = np.random.default_rng(n + count + mode)
    seen = set()
    for bits in ALL_BITS:
        x = _elements(rng, q, n, count, bits, mode)
        want, want_status = model.pack_array(x, q, bits, mode)
        seen |= set(want_status.tolist())
        for offset in (0, 1):
            words, status = _both_forms(torch, ctx, x, bits, mode, offset)
            assert np.array_equal(words, want) and status.tolist() == want_status.tolist(), (bits, offset)
        # decoding what was packed: elements of status 1 come back, truncated fields decode as the model says
        back, back_status = model.unpack_array(want, n, q, bits, mode)
        assert all(np.array_equal(back[e], x[e]) and back_status[e] == 1 for e in range(count) if want_status[e] == 1)
        for offset in (0, 1):
            got, status = _unpack_both_forms(torch, ctx, want, n, bits, mode, offset)
            assert np.array_equal(got, back) and status.tolist() == back_status.tolist(), (bits, offset)
            assert (got < np.uint64(q)).all()
    assert seen == ({1, 0, -1} if count > 3 else {1, 0}), seen
    ctx.close()


@pytest.mark.parametrize("q,n,bits,mode", [(Q14, 64, 15, CENTRED), (Q14, 64, 14, RESIDUE), (Q14, 2, 15, CENTRED), (Q14, 1024, 15, CENTRED), (Q44, 4096, 45, RESIDUE),
                                           (Q60, 128, 63, CENTRED), (Q44, 2, 3, CENTRED), (Q44, 16, 3, RESIDUE)])
def test_unpack_of_a_non_canonical_stream(pkg, q, n, bits, mode):
    """random streams: at these bits some fields lie beyond (q - 1) / 2 (CENTRED) or at q and above (RESIDUE), and at n < 64 the
    padding bits are set; an element of zeros between them stays at status 1"""
    import torch
    count, wpe = 6, model.words(n, bits)
    rng = np.random.default_rng(bits)
    words = rng.integers(0, 2**64, size=(count, wpe), dtype=np.uint64)
    words[2] = 0
    if n * bits % 64:                                            # element 4: valid fields, one padding bit
        words[4] = model.pack_array(np.array([model.in_range_element(rng, n, q, min(bits, 12), mode)], dtype=np.uint64), q, bits, mode)[0][0]
        words[4, -1] |= np.uint64(1 << 63)
    want, want_status = model.unpack_array(words, n, q, bits, mode)
    assert want_status[2] == 1 and want_status[4] == 0
    if n > 2:
        assert want_status[0] == 0 and want_status[1] == 0
    ctx = _context(pkg, q, n)
    for offset in (0, 1):
        got, status = _unpack_both_forms(torch, ctx, words, n, bits, mode, offset)
        assert np.array_equal(got, want) and status.tolist() == want_status.tolist()
        assert (got < np.uint64(q)).all()
    # a status-1 decode is the unique preimage
    ok = want_status == 1
    again, again_status = ctx.ring_pack(want[ok], bits, mode)
    assert np.array_equal(again, words[ok]) and (again_status == 1).all()
    ctx.close()


def test_status_across_workgroups_at_n_65536(pkg):
    """count 2; the only out-of-range coefficient lies in the last 64 of element 0: element 0 is 0 through atomicMin, element 1 stays 1"""
    import torch
    q, n, bits = Q44, 1 << 16, 11
    rng = np.random.default_rng(16)
    x = rng.integers(-1024, 1024, size=(2, n)).astype(np.int64)
    x[0, n - 17] = 1024
    x = np.where(x < 0, x + q, x).astype(np.uint64)
    want, want_status = model.pack_array(x, q, bits, CENTRED)
    assert want_status.tolist() == [0, 1]
    ctx = _context(pkg, q, n)
    words, status = _both_forms(torch, ctx, x, bits, CENTRED)
    assert np.array_equal(words, want) and status.tolist() == [0, 1]
    x[0, n - 17] = q                                            # and -1 the same way
    words, status = _both_forms(torch, ctx, x, bits, CENTRED, offset=1)
    assert status.tolist() == [-1, 1] and np.array_equal(words[1], want[1])
    words = want.copy()
    words[1, -1] |= np.uint64(0x7FF << 53)                      # the last field of element 1 becomes -1
    back, back_status = model.unpack_array(words, n, q, bits, CENTRED)
    got, status = _unpack_both_forms(torch, ctx, words, n, bits, CENTRED)
    assert np.array_equal(got, back) and status.tolist() == back_status.tolist() == [1, 1]
    ctx.close()
    # an invalid field in the last 64 of element 0 of a decode: a modulus below the field's range
    ctx = _context(pkg, Q14, 2048)
    w15 = np.zeros((2, model.words(2048, 15)), dtype=np.uint64)
    w15[0, -1] = np.uint64(0x3FFF << 49)                        # the last field: 2^14 - 1 > (q - 1) / 2
    back, back_status = model.unpack_array(w15, 2048, Q14, 15, CENTRED)
    assert back_status.tolist() == [0, 1]
    got, status = _unpack_both_forms(torch, ctx, w15, 2048, 15, CENTRED)
    assert np.array_equal(got, back) and status.tolist() == [0, 1]
    ctx.close()


def test_overlap_and_alignment_are_refused(pkg):
    import torch
    ctx = _context(pkg, Q44, 64)
    d = torch.zeros(64 * 4, dtype=torch.int64, device="cuda")
    d_s = torch.zeros(4, dtype=torch.int32, device="cuda")
    p = d.data_ptr()
    with pytest.raises(pkg.CoreError, match="out overlaps x"):
        ctx.ring_pack_device(p + 8 * 32, d_s.data_ptr(), p, 1, 11)
    with pytest.raises(pkg.CoreError, match="out overlaps in"):
        ctx.ring_unpack_device(p, d_s.data_ptr(), p + 8 * 10, 1, 11)
    with pytest.raises(pkg.CoreError, match="out overlaps status"):
        ctx.ring_pack_device(p + 8 * 64, p + 8 * 64, p, 1, 11)
    with pytest.raises(pkg.CoreError, match="aligned"):
        ctx.ring_pack_device(p + 8 * 64 + 4, d_s.data_ptr(), p, 1, 11)
    ctx.ring_pack_device(p + 8 * 64, d_s.data_ptr(), p, 1, 11)  # side by side is fine
    torch.cuda.synchronize()
    assert d_s.cpu().tolist()[0] == 1
    ctx.close()


# ---- composition with the existing calls ------------------------------------------------------------------------------------------------------
def test_gadget_digits_pack_at_their_base_and_recompose_after_unpack(pkg):
    q, n, b = Q44, 128, 11
    digits = pkg.ring_gadget_min_digits(q, b)
    ctx = _context(pkg, q, n)
    rng = np.random.default_rng(11)
    x = rng.integers(0, q, size=(5, n), dtype=np.uint64)
    z = ctx.ring_decompose(x, b, digits)
    assert pkg.ring_pack_min_bits(q, CENTRED, 1 << (b - 1)) == b + 1 and pkg.ring_pack_min_bits(q, CENTRED, (1 << (b - 1)) - 1) == b
    words, status = ctx.ring_pack(z.reshape(-1, n), b, CENTRED)
    assert (status == 1).all() and words.shape == (5 * digits, model.words(n, b))
    assert np.array_equal(words, model.pack_array(z.reshape(-1, n), q, b, CENTRED)[0])
    back, status = ctx.ring_unpack(words, b, CENTRED)
    assert (status == 1).all()
    assert np.array_equal(ctx.ring_recompose(back.reshape(5, digits, n), b), x)
    ctx.close()


def test_ball_elements_pack_at_two_bits(pkg):
    q, n = Q44, 256
    ctx = _context(pkg, q, n)
    bits = pkg.ring_pack_min_bits(q, CENTRED, 1)
    assert bits == 2
    x = ctx.ring_sample(9, pkg.RING_SAMPLE_BALL, 60, pkg.ring_sample_key(5))
    words, status = ctx.ring_pack(x, bits, CENTRED)
    assert (status == 1).all() and words.shape == (9, 8)
    assert np.array_equal(words, model.pack_array(x, q, bits, CENTRED)[0])
    back, status = ctx.ring_unpack(words, bits, CENTRED)
    assert (status == 1).all() and np.array_equal(back, x)
    ctx.close()


def test_packed_words_feed_the_transcript_and_the_digests_key_challenges(pkg, lib):
    """pack -> lsr_fs_challenge_batch_device over the packed words (words_per_commitment = width W) -> ring_challenge_device keyed by
    the digests, all on the device; equal to the host route over the model's words"""
    import torch
    q, n, b, messages, width = Q14, 64, 5, 3, 4
    ctx = _context(pkg, q, n)
    rng = np.random.default_rng(3)
    v = rng.integers(-16, 16, size=(messages * width, n))
    x = np.where(v < 0, v + q, v).astype(np.uint64)
    wpe = model.words(n, b)
    s = _stream(torch)
    d_x = _dev(torch, x)
    d_w = torch.zeros((messages, width * wpe), dtype=torch.int64, device="cuda")
    d_s = torch.zeros(messages * width, dtype=torch.int32, device="cuda")
    d_alpha = torch.zeros(messages, dtype=torch.int64, device="cuda")
    d_hash = torch.zeros((messages, 32), dtype=torch.uint8, device="cuda")
    d_c, d_tries = torch.zeros((messages, n), dtype=torch.int64, device="cuda"), torch.zeros(messages, dtype=torch.int32, device="cuda")
    ctx.ring_pack_device(d_w.data_ptr(), d_s.data_ptr(), d_x.data_ptr(), messages * width, b, CENTRED, stream=s)
    assert lib.lsr_fs_challenge_batch_device(None, 0, d_w.data_ptr(), width * wpe, messages, q, d_alpha.data_ptr(), d_hash.data_ptr(), s) == 0
    ctx.ring_challenge_device(d_c.data_ptr(), d_tries.data_ptr(), messages, 31, 10, 15, d_hash.data_ptr(), 1, max_tries=64, stream=s)
    torch.cuda.synchronize()
    assert d_s.cpu().tolist() == [1] * (messages * width)
    want_words = model.pack_array(x, q, b, CENTRED)[0].reshape(messages, width * wpe)
    assert np.array_equal(_host(d_w), want_words)
    digests = [prover_replay.challenge_derive([], want_words[j], q)[1] for j in range(messages)]
    assert [bytes(h) for h in d_hash.cpu().numpy()] == digests
    want, want_tries = ctx.ring_challenge(messages, 31, 10, 15, b"".join(digests), components=1, max_tries=64)
    assert 0 not in want_tries.tolist()
    assert np.array_equal(_host(d_c), want) and d_tries.cpu().tolist() == want_tries.tolist()
    ctx.close()


def test_device_forms_are_captured_on_their_first_call(pkg):
    """no eager call first: a fresh context, pack and unpack (n = 4096: with the status fill kernels) in one graph, replayed twice under
    changed inputs"""
    import torch
    q, n, count, bits = Q44, 4096, 3, 13
    ctx = _context(pkg, q, n)
    wpe = model.words(n, bits)
    rng = np.random.default_rng(9)
    inputs = []
    for k in range(2):
        v = rng.integers(-4096, 4096, size=(count, n))
        v[k, 5 + k] = 4096                                       # the bad element moves
        inputs.append(np.where(v < 0, v + q, v).astype(np.uint64))
    d_x = _dev(torch, inputs[0])
    d_w = torch.zeros((count, wpe), dtype=torch.int64, device="cuda")
    d_back = torch.zeros((count, n), dtype=torch.int64, device="cuda")
    d_s, d_s2 = torch.zeros(count, dtype=torch.int32, device="cuda"), torch.zeros(count, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        s = torch.cuda.current_stream().cuda_stream
        ctx.ring_pack_device(d_w.data_ptr(), d_s.data_ptr(), d_x.data_ptr(), count, bits, CENTRED, stream=s)
        ctx.ring_unpack_device(d_back.data_ptr(), d_s2.data_ptr(), d_w.data_ptr(), count, bits, CENTRED, stream=s)
    for k in (0, 1):
        d_x.copy_(_dev(torch, inputs[k]))
        graph.replay()
        torch.cuda.synchronize()
        want, want_status = model.pack_array(inputs[k], q, bits, CENTRED)
        back, back_status = model.unpack_array(want, n, q, bits, CENTRED)
        assert want_status.tolist() == [0 if e == k else 1 for e in range(count)]
        assert np.array_equal(_host(d_w), want) and d_s.cpu().tolist() == want_status.tolist()
        assert np.array_equal(_host(d_back), back) and d_s2.cpu().tolist() == back_status.tolist() == [1] * count
    ctx.close()
