"""GPU suite: two-prime RNS commitment contexts (lsr_lwe_context_create_rns) against the oracle's single-prime commitments under each
prime and the pure-Python model of tests/rns_model.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import rns_model

pytestmark = pytest.mark.gpu

SIGMA = 3.19
KEY = 77
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ctx(pkg, n, k, sigma=SIGMA, key=KEY):
    return pkg.LweContext.create_rns(pkg.Params(n=n, k=k, sigma=sigma), key_seed=key)


def _split(row, n, k):
    """header, [(u_i [k][n], v_i [n])] of an RNS row"""
    row = np.asarray(row, dtype=np.uint64)
    assert row.size == rns_model.row_words(n, k)
    body = row[rns_model.RNS_HEADER_WORDS:].reshape(2, k + 1, n)
    return [int(x) for x in row[:rns_model.RNS_HEADER_WORDS]], [(body[i, :k], body[i, k]) for i in range(2)]


def _check_row_against_oracle(oracle, row, n, k, msg, seed, sigma=SIGMA, key=KEY):
    q1, q2 = rns_model.rns_moduli(n)
    t = rns_model.plain_modulus(n)
    head, parts = _split(row, n, k)
    assert head == rns_model.header(n, k, t, q1, q2)
    copy = min(len(msg), n)
    for qi, (u, v) in zip((q1, q2), parts):
        want = oracle.lwe_commit(qi, n, k, sigma, key, msg, seed)
        assert int(want[3]) == qi and int(want[4]) == t            # the oracle honours a requested prime of this form
        assert np.array_equal(u.ravel(), want[5:5 + k * n])
        shift = np.zeros(n, dtype=object)
        for x in range(copy):
            shift[x] = (rns_model.message_term(int(msg[x]), t, q1, q2, qi) - rns_model.single_prime_term(int(msg[x]), t, qi)) % qi
        expect = (want[5 + k * n:].astype(object) + shift) % qi
        assert np.array_equal(v.astype(object), expect)


def test_pipeline_names_and_moduli(pkg, lib):
    for n, k, sigma, name in [(4096, 1, SIGMA, "rns-tile"), (4096, 2, SIGMA, "rns-tile"), (4096, 4, SIGMA, "rns-tile"), (1024, 3, SIGMA, "rns-general"),
                              (8192, 2, SIGMA, "rns-general"), (65536, 2, SIGMA, "rns-general"), (4096, 2, 7.5, "rns-general")]:
        ctx = _ctx(pkg, n, k, sigma)
        assert ctx.pipeline == name, (n, k, sigma)
        assert ctx.rns_moduli() == rns_model.rns_moduli(n) == pkg.rns_commit_moduli(n)
        assert ctx.commit_modulus == rns_model.rns_moduli(n)[0] and ctx.plain_modulus == rns_model.plain_modulus(n)
        assert ctx.commitment_words == rns_model.row_words(n, k) and ctx.ring_degree == n and ctx.module_rank == k
        ctx.close()
    plain = pkg.LweContext(pkg.Params(n=4096, k=2, sigma=SIGMA), key_seed=KEY)
    assert plain.rns_moduli() is None and plain.pipeline == "tile"
    plain.close()


@pytest.mark.parametrize("n,k,batch", [(4096, 1, 3), (4096, 2, 5), (4096, 4, 3), (1024, 3, 3), (8192, 2, 3), (65536, 2, 2)])
def test_rows_match_the_oracle_under_each_prime(pkg, oracle, n, k, batch):
    ctx = _ctx(pkg, n, k)
    t = ctx.plain_modulus
    rng = np.random.default_rng(n + k)
    seeds = rng.integers(1, 2**63, size=batch, dtype=np.uint64)
    # ragged batch through the legacy call: lengths 1, n, > n (truncated), with 0, t - 1 and words >= t (embedded mod t)
    lengths = [1, n, n + 3, 7, 2][:batch]
    for j, length in enumerate(lengths):
        msg = rng.integers(0, t, size=length, dtype=np.uint64)
        msg[0] = [0, t - 1, t + 5, 2**64 - 1, 3][j]
        if length > 2:
            msg[1], msg[2] = t - 1, 3 * t + 1
        com = pkg.Commitment.__new__(pkg.Commitment)
        com._lib, com._ctx = ctx._lib, ctx
        com._p = ctx._lib.lwe_commit(ctx.handle, msg.ctypes.data, msg.size, int(seeds[j]))
        assert com._p
        _check_row_against_oracle(oracle, com.as_words(), n, k, msg, int(seeds[j]))
        com.free()
    # a rectangular batch through the flat call
    msgs = rng.integers(0, 2**64, size=(batch, 6), dtype=np.uint64)
    msgs[0, :3] = [0, t - 1, t]
    rows = pkg.Commitment.batch_words(ctx, msgs, seeds)
    for j in range(batch):
        _check_row_against_oracle(oracle, rows[j], n, k, msgs[j], int(seeds[j]))
    ctx.close()


def _device_rows(ctx, msgs, keys, stream=0):
    import torch
    d_msgs = torch.from_numpy(msgs.view(np.int64)).cuda()
    d_keys = torch.from_numpy(keys.view(np.int64)).cuda()
    rows = torch.zeros((msgs.shape[0], ctx.commitment_words), dtype=torch.int64, device="cuda")
    ctx.commit_rows_device(d_msgs.data_ptr(), msgs.shape[1], msgs.shape[0], d_keys.data_ptr(), rows.data_ptr(), stream)
    torch.cuda.synchronize()
    return rows.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("n,k", [(4096, 2), (1024, 3)])
def test_entry_points_agree_word_for_word(pkg, n, k):
    import torch
    ctx = _ctx(pkg, n, k)
    rng = np.random.default_rng(5)
    batch, msg_len = 9, 11
    msgs = rng.integers(0, 2**64, size=(batch, msg_len), dtype=np.uint64)
    seeds = rng.integers(1, 2**63, size=batch, dtype=np.uint64)
    flat = pkg.Commitment.batch_words(ctx, msgs, seeds)
    coms = pkg.Commitment.batch(ctx, msgs, seeds)
    for j in range(batch):
        assert np.array_equal(coms[j].as_words(), flat[j])
        single = ctx._lib.lwe_commit(ctx.handle, msgs[j].ctypes.data, msg_len, int(seeds[j]))
        assert single and single.contents.len == ctx.commitment_words
        assert np.array_equal(np.ctypeslib.as_array(single.contents.data, shape=(single.contents.len,)), flat[j])
        ctx._lib.lwe_commitment_free(single)
    d_out = torch.zeros((batch, ctx.commitment_words), dtype=torch.int64, device="cuda")
    assert ctx._lib.lsr_lwe_commit_batch_flat_device(ctx.handle, msgs.ctypes.data, msg_len, batch, seeds.ctypes.data, d_out.data_ptr()) == 0
    assert np.array_equal(d_out.cpu().numpy().view(np.uint64), flat)
    # keys on the device, then rows on the device
    d_msgs = torch.from_numpy(msgs.view(np.int64)).cuda()
    d_keys = torch.zeros((batch, 4), dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    ctx.commit_keys_device(d_msgs.data_ptr(), msg_len, seeds, d_keys.data_ptr(), s)
    torch.cuda.synchronize()
    keys = ctx.commit_keys(msgs, seeds)
    assert np.array_equal(d_keys.cpu().numpy().view(np.uint64), keys)
    assert np.array_equal(_device_rows(ctx, msgs, keys), flat)
    ctx.close()


_GENERAL_ROWS = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as entry
pkg = entry.load_package()
ctx = pkg.LweContext.create_rns(pkg.Params(n=4096, k=2, sigma=3.19), key_seed=77)
assert ctx.pipeline == sys.argv[3], ctx.pipeline
rng = np.random.default_rng(2048)
msgs = rng.integers(0, 2**64, size=(2048, 9), dtype=np.uint64)
seeds = rng.integers(1, 2**63, size=2048, dtype=np.uint64)
rows = pkg.Commitment.batch_words(ctx, msgs, seeds)
np.save(sys.argv[2], rows)
"""


def test_tile_rows_equal_the_general_composition(pkg, tmp_path):
    """2048 rows at (4096, 2): the single-launch pipeline against the same context's general composition (LAMBDA_SNARK_COMMIT_FUSED=0, read
    once at context creation), each in a fresh child process."""
    script = tmp_path / "rows.py"
    script.write_text(_GENERAL_ROWS)
    out = {}
    for name, flag in (("rns-tile", "1"), ("rns-general", "0")):
        path = str(tmp_path / (name + ".npy"))
        env = dict(os.environ, LAMBDA_SNARK_COMMIT_FUSED=flag)
        subprocess.run([sys.executable, str(script), ROOT, path, name], check=True, env=env, timeout=600)
        out[name] = np.load(path)
    assert out["rns-tile"].shape == (2048, rns_model.row_words(4096, 2))
    assert np.array_equal(out["rns-tile"], out["rns-general"])


def _verify_all(pkg, ctx, rows, msgs):
    """the four verify entry points on [count][words] rows and [count][msg_len] claimed messages -> four verdict lists"""
    import torch
    lib = ctx._lib
    count, msg_len = msgs.shape
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    msgs = np.ascontiguousarray(msgs, dtype=np.uint64)
    views = [pkg._abi.LweCommitment(rows[j].ctypes.data_as(pkg._abi.u64p), rows.shape[1]) for j in range(count)]
    single = [lib.lwe_verify_opening(ctx.handle, ctypes.byref(views[j]), msgs[j].ctypes.data, msg_len, None) for j in range(count)]
    ptrs = (ctypes.POINTER(pkg._abi.LweCommitment) * count)(*[ctypes.pointer(v) for v in views])
    res = np.zeros(count, dtype=np.int32)
    assert lib.lwe_verify_opening_batch(ctx.handle, ptrs, msgs.ctypes.data, msg_len, count, res.ctypes.data) == 0
    batch = res.tolist()
    res2 = np.zeros(count, dtype=np.int32)
    assert lib.lsr_lwe_verify_opening_batch_flat(ctx.handle, rows.ctypes.data, msgs.ctypes.data, msg_len, count, res2.ctypes.data) == 0
    out = [single, batch, res2.tolist()]
    if 1 <= msg_len <= ctx.ring_degree:
        d_rows = torch.from_numpy(rows.view(np.int64)).cuda()
        d_msgs = torch.from_numpy(msgs.view(np.int64)).cuda()
        d_res = torch.zeros(count, dtype=torch.int32, device="cuda")
        ctx.verify_rows_device(d_rows.data_ptr(), d_msgs.data_ptr(), msg_len, count, d_res.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        out.append(d_res.cpu().tolist())
    return out


@pytest.mark.parametrize("n,k", [(4096, 2), (4096, 4), (1024, 3), (8192, 2)])
def test_openings(pkg, n, k):
    ctx = _ctx(pkg, n, k)
    t = ctx.plain_modulus
    q1, q2 = ctx.rns_moduli()
    rng = np.random.default_rng(n * 7 + k)
    count, msg_len = 6, 33
    msgs = rng.integers(0, t, size=(count, msg_len), dtype=np.uint64)
    msgs[0, :3] = [0, t - 1, 1]
    seeds = rng.integers(1, 2**63, size=count, dtype=np.uint64)
    rows = pkg.Commitment.batch_words(ctx, msgs, seeds)
    for verdicts in _verify_all(pkg, ctx, rows, msgs):
        assert verdicts == [1] * count
    full = rng.integers(0, t, size=(2, n), dtype=np.uint64)                 # every slot
    full_rows = pkg.Commitment.batch_words(ctx, full, seeds[:2])
    for verdicts in _verify_all(pkg, ctx, full_rows, full):
        assert verdicts == [1, 1]
    claimed = msgs.copy()
    claimed[1, 5] = (claimed[1, 5] + 1) % t                                  # one changed slot
    claimed[2, 0] += t                                                       # congruent word >= t: compared as given
    claimed[3, msg_len - 1] ^= 1
    for verdicts in _verify_all(pkg, ctx, rows, claimed):
        assert verdicts == [1, 0, 0, 0, 1, 1]
    # defects of the row itself
    block = (k + 1) * n
    bad = np.repeat(rows[:1], 8, axis=0).copy()
    bad[1, 1] ^= 1                                   # magic
    bad[2, 3] = q2                                   # q1 word
    bad[3, 4] = q1                                   # q2 word
    bad[4, 0] -= 8                                   # payload length
    bad[5, 6 + 17] = q1                              # residue word >= q1 in u_1
    bad[6, 6 + block + block - 1] = q2 + 5           # residue word >= q2 in v_2
    bad[7, 6 + block - 1] = 2**63                    # v_1
    for verdicts in _verify_all(pkg, ctx, bad, np.repeat(msgs[:1], 8, axis=0)):
        assert verdicts == [1] + [-1] * 7
    # msg_len > n: 0 on a canonical row, -1 on a non-canonical one (host entry points)
    longmsg = np.zeros((2, n + 1), dtype=np.uint64)
    for verdicts in _verify_all(pkg, ctx, bad[[0, 6]], longmsg):
        assert verdicts == [0, -1]
    # a single-prime row under the RNS context and an RNS row under single-prime contexts
    for q in (q1, q2):
        plain = pkg.LweContext(pkg.Params(q=q, n=n, k=k, sigma=SIGMA), key_seed=KEY)
        assert plain.commit_modulus == q
        prow = pkg.Commitment.batch_words(plain, msgs[:1], seeds[:1])
        padded = np.zeros((1, rows.shape[1]), dtype=np.uint64)
        padded[0, :prow.shape[1]] = prow[0]
        view = pkg._abi.LweCommitment(prow[0].ctypes.data_as(pkg._abi.u64p), prow.shape[1])
        assert ctx._lib.lwe_verify_opening(ctx.handle, ctypes.byref(view), msgs[0].ctypes.data, msg_len, None) == -1
        for verdicts in _verify_all(pkg, ctx, padded, msgs[:1]):
            assert verdicts == [-1]
        rview = pkg._abi.LweCommitment(rows[0].ctypes.data_as(pkg._abi.u64p), rows.shape[1])
        assert ctx._lib.lwe_verify_opening(plain.handle, ctypes.byref(rview), msgs[0].ctypes.data, msg_len, None) == -1
        res = np.zeros(1, dtype=np.int32)
        assert ctx._lib.lsr_lwe_verify_opening_batch_flat(plain.handle, rows[0].ctypes.data, msgs[0].ctypes.data, msg_len, 1, res.ctypes.data) == 0
        assert res[0] == -1
        plain.close()
    ctx.close()


def _combine_model(rows, coeffs, n, k, t, q1, q2):
    block = (k + 1) * n
    acc = [np.zeros(block, dtype=object), np.zeros(block, dtype=object)]
    for row, c in zip(rows, coeffs):
        if row is None:
            continue
        c %= t
        cc = c - t if c > t // 2 else c
        body = np.asarray(row[6:], dtype=np.uint64).astype(object)
        for i, qi in enumerate((q1, q2)):
            acc[i] = (acc[i] + cc * body[i * block:(i + 1) * block]) % qi
    return np.concatenate(acc)


@pytest.mark.parametrize("n,k", [(4096, 2), (1024, 3)])
def test_full_range_linear_combinations(pkg, n, k):
    """The reason for the feature: the sixteen-term, full-range-coefficient case of test_large_combination_coefficients_need_a_wide_modulus
    on an RNS context; the same coefficients on a default context are still refused."""
    ctx = _ctx(pkg, n, k, key=6)
    t = ctx.plain_modulus
    q1, q2 = ctx.rns_moduli()
    rng = np.random.default_rng(60)
    many = [[int(x) for x in rng.integers(0, t, 6)] for _ in range(16)]
    cs = [int(x) for x in rng.integers(0, t, 16)]
    coms = [pkg.Commitment(ctx, m, seed=100 + i) for i, m in enumerate(many)]
    comb = pkg.Commitment.linear_combine(ctx, coms, cs)
    expect = [sum(c * m[i] for c, m in zip(cs, many)) % t for i in range(6)]
    assert pkg.verify_opening_with_context(ctx, comb, expect)
    assert not pkg.verify_opening_with_context(ctx, comb, [(expect[0] + 1) % t] + expect[1:])
    words = comb.as_words()
    assert [int(x) for x in words[:6]] == rns_model.header(n, k, t, q1, q2)
    assert np.array_equal(words[6:].astype(object), _combine_model([c.as_words() for c in coms], cs, n, k, t, q1, q2))
    narrow = pkg.LweContext(pkg.Params(q=17592186044417, n=n, k=k, sigma=SIGMA), key_seed=6)
    ncoms = [pkg.Commitment(narrow, m, seed=100 + i) for i, m in enumerate(many)]
    with pytest.raises(pkg.CoreError):
        pkg.Commitment.linear_combine(narrow, ncoms, cs)
    assert "noise budget" in pkg._abi.last_error()
    narrow.close()
    # NULL entries are skipped; t - 1 acts as -1 and subtracts
    a, b = coms[0], coms[1]
    diff = pkg.Commitment.linear_combine(ctx, [a, None, b], [1, 12345, t - 1])
    assert pkg.verify_opening_with_context(ctx, diff, [(x - y) % t for x, y in zip(many[0], many[1])])
    assert np.array_equal(diff.as_words()[6:].astype(object), _combine_model([a.as_words(), None, b.as_words()], [1, 12345, t - 1], n, k, t, q1, q2))
    # heavier: 1024 terms, coefficients t - 1 or ceil(t / 2), messages t - 1
    base = pkg.Commitment.batch(ctx, np.full((1024, 4), t - 1, dtype=np.uint64), np.arange(1, 1025, dtype=np.uint64))
    heavy_c = [t - 1 if i % 2 else (t + 1) // 2 for i in range(1024)]
    heavy = pkg.Commitment.linear_combine(ctx, base, heavy_c)
    assert pkg.verify_opening_with_context(ctx, heavy, [sum(c * (t - 1) for c in heavy_c) % t] * 4)
    ctx.close()


def test_refusals_name_the_rns_context_and_leave_it_usable(pkg, lib):
    import torch
    ctx = _ctx(pkg, 4096, 2)
    h = ctx.handle
    d = torch.zeros(2 * 4096 * 4, dtype=torch.int64, device="cuda")
    seeds = np.arange(1, 3, dtype=np.uint64)
    s = torch.cuda.current_stream().cuda_stream

    def refused(rc_or_ptr, null=False):
        assert (not rc_or_ptr) if null else rc_or_ptr == -1
        assert b"RNS" in lib.lsr_last_error(), lib.lsr_last_error()

    refused(lib.lsr_mlwe_matvec_batch_device(h, d.data_ptr(), d.data_ptr(), d.data_ptr(), 1, None, s))
    refused(lib.lsr_lwe_sample_blinding_device(h, d.data_ptr(), 1, seeds.ctypes.data, s))
    a = np.zeros((2, 2, 4096), dtype=np.uint64)
    refused(lib.lsr_lwe_public_matrix(h, a.ctypes.data))
    refused(lib.lsr_lwe_ntt_context(h), null=True)
    refused(lib.lsr_lwe_context_replicate(h, -1), null=True)
    handles = (ctypes.c_void_p * 1)(h)
    msgs = np.zeros((2, 4), dtype=np.uint64)
    out = np.zeros((2, ctx.commitment_words), dtype=np.uint64)
    refused(lib.lsr_lwe_commit_batch_flat_sharded(handles, 1, msgs.ctypes.data, 4, 2, seeds.ctypes.data, out.ctypes.data))
    ptr = (ctypes.c_void_p * 1)(d.data_ptr())
    sec = (ctypes.c_double * 2)()
    refused(lib.lsr_mlwe_matvec_batch_sharded(handles, 1, ptr, ptr, 1, out.ctypes.data, sec))
    refused(lib.lsr_mlwe_matvec_batch_sharded_stats(handles, 1, ptr, ptr, 1, out.ctypes.data, sec))
    # the provers and their verifiers
    prover = lib.lsr_simple_prover_create(lib.lsr_prover_modulus(), -1)
    assert prover
    w = np.arange(8, dtype=np.uint64)
    buf = np.zeros(4 * ctx.commitment_words + 64, dtype=np.uint64)
    refused(lib.lsr_simple_prove_batch(prover, h, ctx.commit_modulus, 0, w.ctypes.data, 8, 1, None, 0, seeds.ctypes.data, buf.ctypes.data, buf.ctypes.data,
                                       buf.ctypes.data, buf.ctypes.data, buf.ctypes.data))
    refused(lib.lsr_simple_prove_batch_device(prover, h, ctx.commit_modulus, 0, d.data_ptr(), 8, 1, None, 0, seeds.ctypes.data, d.data_ptr(), d.data_ptr(),
                                              d.data_ptr(), d.data_ptr(), d.data_ptr(), s))
    res = np.zeros(1, dtype=np.int32)
    refused(lib.lsr_simple_verify_batch(lib.lsr_prover_modulus(), None, 0, buf.ctypes.data, ctx.commitment_words, buf.ctypes.data, w.ctypes.data, 8, 1, h,
                                        ctx.commit_modulus, res.ctypes.data))
    refused(lib.lsr_simple_verify_batch_device(lib.lsr_prover_modulus(), None, 0, d.data_ptr(), ctx.commitment_words, d.data_ptr(), d.data_ptr(), 8, 1, h,
                                               ctx.commit_modulus, d.data_ptr(), s))
    lib.lsr_simple_prover_free(prover)
    ent = (pkg._abi.SparseEntry * 1)(pkg._abi.SparseEntry(0, 0, 1))
    mat = pkg._abi.SparseMatrix(ent, 1, 4, 4)
    r1 = lib.lsr_r1cs_prover_create(ctypes.byref(mat), ctypes.byref(mat), ctypes.byref(mat), -1)
    assert r1
    st = np.zeros(4, dtype=np.uint32)
    refused(lib.lsr_r1cs_prove_batch(r1, h, ctx.commit_modulus, w.ctypes.data, 1, 1, seeds.ctypes.data, None, buf.ctypes.data, buf.ctypes.data, None,
                                     st.ctypes.data))
    refused(lib.lsr_r1cs_prove_batch_device(r1, h, ctx.commit_modulus, d.data_ptr(), 1, 1, seeds.ctypes.data, None, d.data_ptr(), d.data_ptr(), None,
                                            d.data_ptr(), s))
    lib.lsr_r1cs_prover_free(r1)
    # still usable
    com = pkg.Commitment(ctx, [1, 2, 3], seed=9)
    assert pkg.verify_opening_with_context(ctx, com, [1, 2, 3])
    ctx.close()


@pytest.mark.parametrize("n,k", [(4096, 2), (8192, 2)])
def test_asynchronous_calls_on_one_context_are_ordered(pkg, n, k):
    """Two asynchronous commit_rows_device calls on two streams on one context (shared workspaces) give the rows of sequential calls."""
    import torch
    ctx = _ctx(pkg, n, k)
    rng = np.random.default_rng(11)
    batch, msg_len = 40, 5
    sets = []
    for _ in range(2):
        msgs = rng.integers(0, ctx.plain_modulus, size=(batch, msg_len), dtype=np.uint64)
        seeds = rng.integers(1, 2**63, size=batch, dtype=np.uint64)
        keys = ctx.commit_keys(msgs, seeds)
        sets.append((msgs, keys, _device_rows(ctx, msgs, keys)))
    d_in = [(torch.from_numpy(m.view(np.int64)).cuda(), torch.from_numpy(kk.view(np.int64)).cuda()) for m, kk, _ in sets]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for it in range(10):
        outs = [torch.zeros((batch, ctx.commitment_words), dtype=torch.int64, device="cuda") for _ in range(2)]
        res = torch.zeros(batch, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for i in range(2):
            ctx.commit_rows_device(d_in[i][0].data_ptr(), msg_len, batch, d_in[i][1].data_ptr(), outs[i].data_ptr(), streams[i].cuda_stream)
        ctx.verify_rows_device(outs[1].data_ptr(), d_in[1][0].data_ptr(), msg_len, batch, res.data_ptr(), streams[0].cuda_stream)
        torch.cuda.synchronize()
        for i in range(2):
            assert np.array_equal(outs[i].cpu().numpy().view(np.uint64), sets[i][2]), (it, i)
        assert int(res.sum().item()) == batch, it
    ctx.close()
