"""GPU suite: the wavefront-cooperative transcript kernel (WAVE), the lane kernel (LANE) and the rule that picks between them (AUTO)
against hashlib's SHA3-256 over the transcript of challenge.rs:102-134, single and chained (alpha -> beta), word for word."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

AUTO, LANE, WAVE = 0, 1, 2
N_INPUTS = [0, 1, 2, 14, 15, 16, 17, 40]
ROW_WORDS = [1, 2, 13, 14, 15, 16, 17, 31, 33, 34, 100, 12293]
COUNTS = [1, 2, 3, 7, 8, 9, 63, 64, 65, 1000]      # WAVE: 2 transcripts per wavefront = per workgroup; LANE: 64
MODULI = [12289, 17592186044417, 2**64 - 2**32 + 1]
U64 = 2**64 - 1


def derive(inputs, words, modulus):
    h = hashlib.sha3_256(b"LAMBDA-SNARK-R-FS-v1")
    h.update(len(inputs).to_bytes(8, "little"))
    h.update(np.asarray(inputs, dtype="<u8").tobytes())
    h.update(len(words).to_bytes(8, "little"))
    h.update(np.asarray(words, dtype="<u8").tobytes())
    digest = h.digest()
    return int.from_bytes(digest[:8], "little"), digest


def expected(ins, rows):
    """Per row: the raw 64-bit words and digests of both transcripts are modulus-dependent through alpha, so return a function."""
    firsts = [derive(ins[i], rows[i], 1) for i in range(len(rows))]

    def for_modulus(modulus):
        al = np.array([w % modulus for w, _ in firsts], dtype=np.uint64)
        second = [derive([int(a)], rows[i], 1) for i, a in enumerate(al)]
        be = np.array([w % modulus for w, _ in second], dtype=np.uint64)
        ha = np.frombuffer(b"".join(d for _, d in firsts), dtype=np.uint8).reshape(-1, 32)
        hb = np.frombuffer(b"".join(d for _, d in second), dtype=np.uint8).reshape(-1, 32)
        return al, be, ha, hb
    return for_modulus


def make(rng, count, row_words, n_inputs, modulus=17592186044417):
    rows = rng.integers(0, 2**64, size=(count, row_words), dtype=np.uint64)
    ins = rng.integers(0, 2**64, size=(count, max(n_inputs, 1)), dtype=np.uint64)
    rows.reshape(-1)[::7] %= np.uint64(modulus)
    ins.reshape(-1)[::3] %= np.uint64(modulus)
    rows[0, 0] = np.uint64(U64)
    return rows, np.ascontiguousarray(ins[:, :n_inputs])


def to_dev(a):
    import torch
    return torch.from_numpy(a.view(np.int64).copy()).cuda()


def u64(t):
    return t.cpu().numpy().view(np.uint64)


class Out:
    def __init__(self, count):
        import torch
        self.al = torch.full((count,), -1, dtype=torch.int64, device="cuda")
        self.be = torch.full((count,), -1, dtype=torch.int64, device="cuda")
        self.ha = torch.full((count, 32), 0xEE, dtype=torch.uint8, device="cuda")
        self.hb = torch.full((count, 32), 0xEE, dtype=torch.uint8, device="cuda")


def counts_for(row_words):
    return [c for c in COUNTS if c <= 65] if row_words > 1000 else COUNTS


@pytest.mark.parametrize("row_words", ROW_WORDS)
@pytest.mark.parametrize("path", [WAVE, LANE])
def test_single_on_each_path_matches_hashlib(lib, path, row_words):
    import torch
    s = torch.cuda.current_stream().cuda_stream
    top = max(counts_for(row_words))
    for n_inputs in N_INPUTS:
        rng = np.random.default_rng(row_words * 977 + n_inputs)
        rows, ins = make(rng, top, row_words, n_inputs)
        want = expected(ins, rows)
        d_rows, d_ins = to_dev(rows), (to_dev(ins) if n_inputs else None)
        p_in = d_ins.data_ptr() if n_inputs else None
        for ci, count in enumerate(counts_for(row_words)):
            modulus = MODULI[(ci + n_inputs) % 3]
            al, _, ha, _ = want(modulus)
            o = Out(top)
            assert lib.lsr_fs_challenge_batch_device_on(path, p_in, n_inputs, d_rows.data_ptr(), row_words, count, modulus, o.al.data_ptr(), o.ha.data_ptr(), s) == 0
            torch.cuda.synchronize()
            assert np.array_equal(u64(o.al)[:count], al[:count]), (path, row_words, n_inputs, count)
            assert np.array_equal(o.ha.cpu().numpy()[:count], ha[:count]), (path, row_words, n_inputs, count)
            assert (u64(o.al)[count:] == U64).all() and (o.ha.cpu().numpy()[count:] == 0xEE).all(), "nothing past `count` is written"
            o = Out(top)
            assert lib.lsr_fs_challenge_batch_device_on(path, p_in, n_inputs, d_rows.data_ptr(), row_words, count, modulus, o.al.data_ptr(), None, s) == 0
            torch.cuda.synchronize()
            assert np.array_equal(u64(o.al)[:count], al[:count]), (path, row_words, n_inputs, count, "no digests")


@pytest.mark.parametrize("row_words", ROW_WORDS)
def test_chain_on_every_path_matches_hashlib_and_two_single_calls(lib, row_words):
    import torch
    s = torch.cuda.current_stream().cuda_stream
    counts = [1, 9, 65] if row_words > 1000 else [1, 2, 9, 64, 65, 1000]
    top = max(counts)
    for n_inputs in N_INPUTS:
        rng = np.random.default_rng(row_words * 613 + n_inputs)
        rows, ins = make(rng, top, row_words, n_inputs)
        want = expected(ins, rows)
        d_rows, d_ins = to_dev(rows), (to_dev(ins) if n_inputs else None)
        p_in = d_ins.data_ptr() if n_inputs else None
        for ci, count in enumerate(counts):
            modulus = MODULI[(ci + n_inputs + 1) % 3]
            al, be, ha, hb = want(modulus)
            for path in (WAVE, LANE, AUTO):
                o = Out(top)
                assert lib.lsr_fs_challenge_chain_batch_device(path, p_in, n_inputs, d_rows.data_ptr(), row_words, count, modulus, o.al.data_ptr(),
                                                               o.be.data_ptr(), o.ha.data_ptr(), o.hb.data_ptr(), s) == 0
                torch.cuda.synchronize()
                where = (path, row_words, n_inputs, count)
                assert np.array_equal(u64(o.al)[:count], al[:count]) and np.array_equal(u64(o.be)[:count], be[:count]), where
                assert np.array_equal(o.ha.cpu().numpy()[:count], ha[:count]) and np.array_equal(o.hb.cpu().numpy()[:count], hb[:count]), where
                assert (u64(o.al)[count:] == U64).all() and (u64(o.be)[count:] == U64).all() and (o.hb.cpu().numpy()[count:] == 0xEE).all(), where
                # digests optional, each on its own
                o2 = Out(top)
                assert lib.lsr_fs_challenge_chain_batch_device(path, p_in, n_inputs, d_rows.data_ptr(), row_words, count, modulus, o2.al.data_ptr(),
                                                               o2.be.data_ptr(), None, o2.hb.data_ptr(), s) == 0
                torch.cuda.synchronize()
                assert torch.equal(o2.al, o.al) and torch.equal(o2.be, o.be) and torch.equal(o2.hb, o.hb), where
            # two single calls, the second fed the first one's device array
            o = Out(top)
            for path in (WAVE, LANE):
                assert lib.lsr_fs_challenge_batch_device_on(path, p_in, n_inputs, d_rows.data_ptr(), row_words, count, modulus, o.al.data_ptr(), o.ha.data_ptr(), s) == 0
                assert lib.lsr_fs_challenge_batch_device_on(path, o.al.data_ptr(), 1, d_rows.data_ptr(), row_words, count, modulus, o.be.data_ptr(), o.hb.data_ptr(), s) == 0
                torch.cuda.synchronize()
                assert np.array_equal(u64(o.be)[:count], be[:count]) and np.array_equal(o.hb.cpu().numpy()[:count], hb[:count]), (path, row_words, n_inputs, count)


def test_chain_over_real_wire_rows_at_reference_size(pkg, lib):
    """512 rows of 12 293 words produced on the device by lsr_lwe_commit_batch_flat_device, never leaving it before they are hashed."""
    import torch
    q, n, k = 17592186044417, 4096, 2
    ctx = pkg.LweContext(pkg.Params(q=q, n=n, k=k, sigma=3.19), key_seed=0xFEED)
    batch, W = 512, lib.lsr_lwe_commitment_words(ctx.handle)
    assert W == 12293
    rng = np.random.default_rng(99)
    msgs = rng.integers(0, 2**20, size=(batch, 7), dtype=np.uint64)
    seeds = rng.integers(1, 2**62, size=batch, dtype=np.uint64)
    publics = rng.integers(0, 2**44, size=(batch, 2), dtype=np.uint64)
    d_rows = torch.zeros((batch, W), dtype=torch.int64, device="cuda")
    assert lib.lsr_lwe_commit_batch_flat_device(ctx.handle, msgs.ctypes.data, 7, batch, seeds.ctypes.data, d_rows.data_ptr()) == 0
    torch.cuda.synchronize()
    d_pub = to_dev(publics)
    s = torch.cuda.current_stream().cuda_stream
    al, be, ha, hb = expected(publics, u64(d_rows))(q)
    for path in (WAVE, LANE, AUTO):
        o = Out(batch)
        assert lib.lsr_fs_challenge_chain_batch_device(path, d_pub.data_ptr(), 2, d_rows.data_ptr(), W, batch, q, o.al.data_ptr(), o.be.data_ptr(),
                                                       o.ha.data_ptr(), o.hb.data_ptr(), s) == 0
        torch.cuda.synchronize()
        assert np.array_equal(u64(o.al), al) and np.array_equal(u64(o.be), be), path
        assert np.array_equal(o.ha.cpu().numpy(), ha) and np.array_equal(o.hb.cpu().numpy(), hb), path
    ctx.close()


def test_auto_equals_both_paths_on_either_side_of_the_switch(lib):
    """The switch point is asked of lsr_fs_transcript_path, not restated: the largest count that still goes to WAVE, and the next."""
    import torch
    W, n_inputs, q = 34, 2, 17592186044417
    lo, hi = 1, 2**26
    assert lib.lsr_fs_transcript_path(lo, W) == WAVE and lib.lsr_fs_transcript_path(hi, W) == LANE
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if lib.lsr_fs_transcript_path(mid, W) == WAVE:
            lo = mid
        else:
            hi = mid
    assert lo < 2**22, "a switch point that the test can afford to hash"
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    d_rows = torch.randint(-2**63, 2**63 - 1, (hi, W), dtype=torch.int64, device="cuda", generator=g)
    d_ins = torch.randint(-2**63, 2**63 - 1, (hi, n_inputs), dtype=torch.int64, device="cuda", generator=g)
    rows, ins = u64(d_rows), u64(d_ins)
    probe = [0, 1, lo - 1, hi - 1]
    for count, picked in ((lo, WAVE), (hi, LANE)):
        assert lib.lsr_fs_transcript_path(count, W) == picked
        outs = {}
        for path in (AUTO, LANE, WAVE):
            o = Out(count)
            assert lib.lsr_fs_challenge_chain_batch_device(path, d_ins.data_ptr(), n_inputs, d_rows.data_ptr(), W, count, q, o.al.data_ptr(), o.be.data_ptr(),
                                                           o.ha.data_ptr(), o.hb.data_ptr(), s) == 0
            o1 = Out(count)
            assert lib.lsr_fs_challenge_batch_device_on(path, d_ins.data_ptr(), n_inputs, d_rows.data_ptr(), W, count, q, o1.al.data_ptr(), o1.ha.data_ptr(), s) == 0
            torch.cuda.synchronize()
            assert torch.equal(o.al, o1.al) and torch.equal(o.ha, o1.ha)
            outs[path] = o
        old = Out(count)     # the unchanged entry point is AUTO
        assert lib.lsr_fs_challenge_batch_device(d_ins.data_ptr(), n_inputs, d_rows.data_ptr(), W, count, q, old.al.data_ptr(), old.ha.data_ptr(), s) == 0
        torch.cuda.synchronize()
        for path in (LANE, WAVE):
            for name in ("al", "be", "ha", "hb"):
                assert torch.equal(getattr(outs[AUTO], name), getattr(outs[path], name)), (count, path, name)
        assert torch.equal(old.al, outs[AUTO].al) and torch.equal(old.ha, outs[AUTO].ha)
        al, be = u64(outs[AUTO].al), u64(outs[AUTO].be)
        for i in probe:
            if i < count:
                a, _ = derive(ins[i], rows[i], 1)
                b, _ = derive([a % q], rows[i], 1)
                assert (int(al[i]), int(be[i])) == (a % q, b % q), (count, i)


def test_two_streams_at_once(lib):
    import torch
    W, n_inputs, count, q = 12293, 2, 64, 17592186044417
    sets = []
    for k in range(2):
        rows, ins = make(np.random.default_rng(40 + k), count, W, n_inputs)
        sets.append((rows, ins, to_dev(rows), to_dev(ins), Out(count), torch.cuda.Stream()))
    torch.cuda.synchronize()
    for _ in range(3):
        for rows, ins, d_rows, d_ins, o, st in sets:
            assert lib.lsr_fs_challenge_chain_batch_device(WAVE, d_ins.data_ptr(), n_inputs, d_rows.data_ptr(), W, count, q, o.al.data_ptr(), o.be.data_ptr(),
                                                           o.ha.data_ptr(), o.hb.data_ptr(), st.cuda_stream) == 0
    torch.cuda.synchronize()
    for rows, ins, d_rows, d_ins, o, st in sets:
        al, be, ha, hb = expected(ins, rows)(q)
        assert np.array_equal(u64(o.al), al) and np.array_equal(u64(o.be), be)
        assert np.array_equal(o.ha.cpu().numpy(), ha) and np.array_equal(o.hb.cpu().numpy(), hb)


def test_wave_chain_captured_into_a_graph_replays_three_times(lib):
    import torch
    W, n_inputs, count, q = 300, 3, 37, 17592186044417
    rows, ins = make(np.random.default_rng(77), count, W, n_inputs)
    d_rows, d_ins, o = to_dev(rows), to_dev(ins), Out(count)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        assert lib.lsr_fs_challenge_chain_batch_device(WAVE, d_ins.data_ptr(), n_inputs, d_rows.data_ptr(), W, count, q, o.al.data_ptr(), o.be.data_ptr(),
                                                       o.ha.data_ptr(), o.hb.data_ptr(), side.cuda_stream) == 0
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        rc = lib.lsr_fs_challenge_chain_batch_device(WAVE, d_ins.data_ptr(), n_inputs, d_rows.data_ptr(), W, count, q, o.al.data_ptr(), o.be.data_ptr(),
                                                     o.ha.data_ptr(), o.hb.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    for replay in range(3):
        # new inputs in the captured buffers each time, outputs wiped: a replay that did nothing cannot pass
        rows, ins = make(np.random.default_rng(100 + replay), count, W, n_inputs)
        d_rows.copy_(to_dev(rows)); d_ins.copy_(to_dev(ins))
        o.al.fill_(-1); o.be.fill_(-1); o.ha.fill_(0xEE); o.hb.fill_(0xEE)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        al, be, ha, hb = expected(ins, rows)(q)
        assert np.array_equal(u64(o.al), al) and np.array_equal(u64(o.be), be), replay
        assert np.array_equal(o.ha.cpu().numpy(), ha) and np.array_equal(o.hb.cpu().numpy(), hb), replay


def test_device_argument_contract(lib, pkg):
    import torch
    d = torch.zeros(64, dtype=torch.int64, device="cuda")
    P, s = d.data_ptr(), torch.cuda.current_stream().cuda_stream
    single, chain = lib.lsr_fs_challenge_batch_device_on, lib.lsr_fs_challenge_chain_batch_device
    for path in (AUTO, LANE, WAVE):
        assert single(path, None, 2, P, 4, 2, 12289, P + 256, None, s) == -1
        assert single(path, None, 0, None, 4, 2, 12289, P + 256, None, s) == -1
        assert single(path, None, 0, P, 0, 2, 12289, P + 256, None, s) == -1
        assert single(path, None, 0, P, 4, 2, 0, P + 256, None, s) == -1
        assert single(path, None, 0, P, 4, 2, 12289, None, None, s) == -1
        assert single(path, None, 0, P, 4, 0, 12289, P + 256, None, s) == 0
        assert single(path, None, 0, P, 4, 2, 12289, P + 256, None, s) == 0
        assert chain(path, None, 2, P, 4, 2, 12289, P + 256, P + 384, None, None, s) == -1
        assert chain(path, None, 0, None, 4, 2, 12289, P + 256, P + 384, None, None, s) == -1
        assert chain(path, None, 0, P, 0, 2, 12289, P + 256, P + 384, None, None, s) == -1
        assert chain(path, None, 0, P, 4, 2, 0, P + 256, P + 384, None, None, s) == -1
        assert chain(path, None, 0, P, 4, 2, 12289, None, P + 384, None, None, s) == -1
        assert chain(path, None, 0, P, 4, 2, 12289, P + 256, None, None, None, s) == -1
        assert chain(path, None, 0, P, 4, 0, 12289, P + 256, P + 384, None, None, s) == 0
        assert chain(path, None, 0, P, 4, 2, 12289, P + 256, P + 384, None, None, s) == 0
    for path in (3, -1, 99):
        assert single(path, None, 0, P, 4, 2, 12289, P + 256, None, s) == -1
        assert "path" in pkg._abi.last_error()
        assert chain(path, None, 0, P, 4, 2, 12289, P + 256, P + 384, None, None, s) == -1
        assert "path" in pkg._abi.last_error()
    torch.cuda.synchronize()
    zero_rows = np.zeros((2, 4), dtype=np.uint64)
    a, _ = derive([], zero_rows[0], 1)
    assert int(u64(d)[32]) == a % 12289 and int(u64(d)[33]) == a % 12289
