"""GPU suite: the commitment kernels at every module rank.  The one-workgroup kernels at n = 4096 are templates over the rank K — its
own f8_tile_pipeline, matrix layout, LDS image (keep[(2K + 1) 4096]), register budget and row addressing (v at K 4096 words, the
second prime's block at (K + 1) 4096) — dispatched through for_rank in lsr_commit.hip; this suite launches every one of them, on
default and on two-prime contexts, and the fused pipeline's decode and openings at the ranks the other suites leave out.

    kernel                              ranks some test launches                                   never launched
    commit_tile_kernel<K>               1, 2, 3, 4 (test_commit_rows_gpu, here)                    none
    verify_tile_kernel<K>               2 (many), 4 (test_sampler_regimes_gpu); 1, 2, 3, 4 here    none
    decode_tile_kernel<K, NOISE>        1, 2, 4 (test_decode_gpu); 1, 2, 3, 4 here, both NOISE     none
    commit_rns_tile_kernel<K>           1, 2, 4 (test_rns_commit_gpu); 1, 2, 3, 4 here             none
    verify_rns_tile_kernel<K>           1, 2, 4; 1, 2, 3, 4 here                                   none
    decode_rns_tile_kernel<K, NOISE>    2, 4; 1, 2, 3, 4 here, both NOISE                          none
    decode_top_inverse_kernel<R, NOISE> (65536, 2), (131072, 1); here (65536, 1 / 3 / 4), (131072, 3), both NOISE
    openings at n = 131072              k = 2, 4; here k = 1, 3

Every comparison is between integers and exact.  Rows are held word for word to the CPU oracle's commitments (under each prime for a
two-prime context).  Decoded slots AND the noise level are held to the big-integer model of tests/decode_model.py evaluated on the
oracle's opening w = v - <s, u> (oracle_lwe_open; for a two-prime row: under each prime on that prime's block re-wrapped as a
single-prime row, then rns_model.crt_lift) — the secret-dependent part of decoding, which is what depends on the rank.  The model's
slots are first asserted equal to the embedded message, so a mismatch of the keys cannot pass as a kernel result."""
import ctypes

import numpy as np
import pytest

import decode_model
import rns_model
from test_rns_commit_gpu import _check_row_against_oracle, _device_rows, _split

pytestmark = pytest.mark.gpu

SIGMA = 3.19
KEY = 77                                   # (the key of test_rns_commit_gpu, which _check_row_against_oracle assumes)
Q_DEFAULT = 17592169062401
SINGLE_MAGIC = int.from_bytes(b"LSRC0001", "little")
SENTINEL = 0x5A5A5A5A5A5A5A5A
VERDICT_SENTINEL = 7


def _context(pkg, kind, n, k, q=Q_DEFAULT):
    params = pkg.Params(n=n, k=k, sigma=SIGMA) if kind == "rns" else pkg.Params(q=q, n=n, k=k, sigma=SIGMA)
    return pkg.LweContext.create_rns(params, key_seed=KEY) if kind == "rns" else pkg.LweContext(params, key_seed=KEY)


def _moduli(ctx):
    return ctx.rns_moduli() or (ctx.commit_modulus,)


def _head(ctx):
    return rns_model.RNS_HEADER_WORDS if ctx.rns_moduli() else 5


def _single_prime_row(n, k, t, qi, u, v):
    """a prime's block of a two-prime row under the header of the oracle's single-prime rows"""
    head = np.array([8 * (4 + (k + 1) * n), SINGLE_MAGIC, n | (k << 32), qi, t], dtype=np.uint64)
    return np.concatenate([head, np.asarray(u, dtype=np.uint64).ravel(), np.asarray(v, dtype=np.uint64)])


def _model(oracle, ctx, row):
    """(slots [n] uint64, noise_bits) of a well-formed row: decode_model.slot_and_rho on the oracle's opening"""
    n, k, t = ctx.ring_degree, ctx.module_rank, ctx.plain_modulus
    pair = ctx.rns_moduli()
    if pair is None:
        big = ctx.commit_modulus
        rc, w = oracle.lwe_open(big, n, k, SIGMA, KEY, row)
        assert rc == 0
        xs = w.tolist()
    else:
        q1, q2 = pair
        big = q1 * q2
        head, parts = _split(row, n, k)
        assert head == rns_model.header(n, k, t, q1, q2)
        residues = []
        for qi, (u, v) in zip(pair, parts):
            rc, w = oracle.lwe_open(qi, n, k, SIGMA, KEY, _single_prime_row(n, k, t, qi, u, v))
            assert rc == 0
            residues.append(w.tolist())
        xs = [rns_model.crt_lift(a, b, q1, q2) for a, b in zip(*residues)]
    pairs = [decode_model.slot_and_rho(x, t, big) for x in xs]
    return np.array([s for s, _ in pairs], dtype=np.uint64), max(r for _, r in pairs).bit_length()


def _models(oracle, ctx, rows, msgs):
    """the models of fresh rows of msgs [batch][msg_len], after asserting that they decode to the embedded message and 0 beyond it"""
    t, moduli = ctx.plain_modulus, _moduli(ctx)
    capacity = decode_model.capacity_bits(moduli[0] * moduli[-1] if len(moduli) == 2 else moduli[0])
    assert capacity == ctx.noise_capacity_bits
    slots, bits = [], []
    for row, msg in zip(rows, msgs):
        s, b = _model(oracle, ctx, row)
        assert np.array_equal(s[:msg.size], msg % np.uint64(t)) and not s[msg.size:].any(), "the model does not open this row: keys or layout differ"
        assert 0 < b < capacity                                                # a fresh row has noise, and headroom
        slots.append(s)
        bits.append(b)
    return np.stack(slots), bits


def _commit_device(ctx, msgs, seeds):
    """commit_rows_device from commit_keys into a buffer one row longer than the call needs, pre-filled: the last row comes back untouched"""
    import torch
    batch, msg_len = msgs.shape
    keys = ctx.commit_keys(msgs, seeds)
    d_msgs = torch.from_numpy(msgs.view(np.int64)).cuda()
    d_keys = torch.from_numpy(keys.view(np.int64)).cuda()
    d_rows = torch.full((batch + 1, ctx.commitment_words), SENTINEL, dtype=torch.int64, device="cuda")
    ctx.commit_rows_device(d_msgs.data_ptr(), msg_len, batch, d_keys.data_ptr(), d_rows.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    rows = d_rows.cpu().numpy().view(np.uint64)
    assert (rows[batch] == np.uint64(SENTINEL)).all(), "the row behind the batch was written"
    return rows[:batch]


def _verify_device(ctx, rows, claimed):
    """verify_rows_device; the verdict buffer is pre-filled and one entry longer than count"""
    import torch
    count, msg_len = claimed.shape
    d_rows = torch.from_numpy(np.ascontiguousarray(rows).view(np.int64)).cuda()
    d_msgs = torch.from_numpy(np.ascontiguousarray(claimed).view(np.int64)).cuda()
    d_res = torch.full((count + 1,), VERDICT_SENTINEL, dtype=torch.int32, device="cuda")
    ctx.verify_rows_device(d_rows.data_ptr(), d_msgs.data_ptr(), msg_len, count, d_res.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    res = d_res.cpu().tolist()
    assert res[count] == VERDICT_SENTINEL, "the verdict behind the batch was written"
    assert np.array_equal(d_rows.cpu().numpy().view(np.uint64), rows), "the rows were written"
    return res[:count]


def _decode_device(ctx, rows, slots, noise):
    """decode_rows_device -> (messages, status, noise_bits or None); every output pre-filled and one entry longer than count"""
    import torch
    count = rows.shape[0]
    d_rows = torch.from_numpy(np.ascontiguousarray(rows).view(np.int64)).cuda()
    d_msgs = torch.full((count + 1, slots), SENTINEL, dtype=torch.int64, device="cuda")
    d_status = torch.full((count + 1,), VERDICT_SENTINEL, dtype=torch.int32, device="cuda")
    d_bits = torch.full((count + 1,), 77, dtype=torch.int32, device="cuda")
    ctx.decode_rows_device(d_rows.data_ptr(), count, slots, d_msgs.data_ptr(), d_status.data_ptr(), d_bits.data_ptr() if noise else None,
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    msgs, status, bits = d_msgs.cpu().numpy().view(np.uint64), d_status.cpu().numpy(), d_bits.cpu().numpy().view(np.uint32)
    assert (msgs[count] == np.uint64(SENTINEL)).all() and status[count] == VERDICT_SENTINEL and bits[count] == 77, "an output was written behind the batch"
    if not noise:
        assert (bits == 77).all(), "the noise output was written without being given"
    return msgs[:count], status[:count], bits[:count] if noise else None


def _messages(rng, t, batch, msg_len):
    msgs = rng.integers(0, t, size=(batch, msg_len), dtype=np.uint64)
    msgs[0, :3] = [2**63 + 5, t, 2**64 - 1]                    # embedded mod t
    return msgs


def _tamper_matrix(ctx, row, msg):
    """(rows, claims, verdicts, the indices of the malformed rows) from one fresh row and its message"""
    n, k, t = ctx.ring_degree, ctx.module_rank, ctx.plain_modulus
    moduli, head, block = _moduli(ctx), _head(ctx), (ctx.module_rank + 1) * ctx.ring_degree
    embedded = msg % np.uint64(t)
    rows, claims, verdicts = [], [], []

    def add(verdict, claim=embedded, index=None, word=None):
        r = row.copy()
        if index is not None:
            r[index] = word
        rows.append(r)
        claims.append(claim)
        verdicts.append(verdict)

    add(1)                                                                     # untouched, the embedded words
    add(0, claim=msg)                                                          # the words >= t as given: compared raw
    wrong = embedded.copy()
    wrong[-1] = (int(wrong[-1]) + 1) % t
    add(0, claim=wrong)                                                        # wrong only in the last slot
    congruent = embedded.copy()
    congruent[0] += np.uint64(t)
    add(0, claim=congruent)                                                    # congruent mod t in slot 0
    add(-1, index=2, word=int(row[2]) ^ (1 << 32))                             # a changed header word: the rank
    for i, qi in enumerate(moduli):                                            # each prime's block at its own modulus
        base = head + i * block
        add(-1, index=base + (k - 1) * n + n - 1, word=qi)                     # coefficient n - 1 of the LAST u polynomial
        add(-1, index=base, word=qi)                                           # coefficient 0 of u_0
        add(-1, index=base + k * n + n - 1, word=qi + 5)                       # a v word >= q in coefficient n - 1
    return np.stack(rows), np.stack(claims), verdicts, [j for j, v in enumerate(verdicts) if v == -1]


def _opening_single(pkg, ctx, row, claim):
    row, claim = np.ascontiguousarray(row), np.ascontiguousarray(claim)
    view = pkg._abi.LweCommitment(row.ctypes.data_as(pkg._abi.u64p), row.size)
    return ctx._lib.lwe_verify_opening(ctx.handle, ctypes.byref(view), claim.ctypes.data, claim.size, None)


@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", ["default", "rns"])
def test_every_rank_on_the_one_workgroup_kernels(pkg, oracle, kind, k):
    n, batch = 4096, 3
    ctx = _context(pkg, kind, n, k)
    try:
        assert ctx.pipeline == ("rns-tile" if kind == "rns" else "tile")         # not the general kernels
        t, moduli = ctx.plain_modulus, _moduli(ctx)
        assert (ctx.commit_modulus == Q_DEFAULT) and ctx.ring_degree == n and ctx.module_rank == k
        rng = np.random.default_rng(1000 * k + (kind == "rns"))
        fresh = {}
        # ---- 1. commit -------------------------------------------------------------------------------------------------------------
        for msg_len in (5, n):
            msgs = _messages(rng, t, batch, msg_len)
            seeds = rng.integers(1, 2**63, size=batch, dtype=np.uint64)
            rows = _commit_device(ctx, msgs, seeds)
            for j in range(batch):
                if kind == "rns":
                    _check_row_against_oracle(oracle, rows[j], n, k, msgs[j], int(seeds[j]))
                else:
                    want = oracle.lwe_commit(Q_DEFAULT, n, k, SIGMA, KEY, [int(x) for x in msgs[j]], int(seeds[j]))
                    assert np.array_equal(rows[j], want), (k, msg_len, j, np.argwhere(rows[j] != want)[:8].tolist())
            fresh[msg_len] = (msgs, rows, _models(oracle, ctx, rows, msgs))
        # ---- 2. verify -------------------------------------------------------------------------------------------------------------
        malformed = {}
        for msg_len in (5, n):
            msgs, rows, _ = fresh[msg_len]
            t_rows, claims, verdicts, bad = _tamper_matrix(ctx, rows[0], msgs[0])
            assert verdicts == [1, 0, 0, 0, -1] + [-1] * (3 * len(moduli))
            if kind == "rns":
                # the smaller prime's value in coefficient n - 1 of v in the larger prime's block: canonical there, so the row is not
                # malformed — it opens to whatever the changed coefficient decodes to, which the model says
                small, large = min(moduli), max(moduli)
                index = _head(ctx) + moduli.index(large) * (k + 1) * n + k * n + n - 1
                extra = rows[0].copy()
                extra[index] = small
                slots, _ = _model(oracle, ctx, extra)
                claim = msgs[0] % np.uint64(t)
                opens = int(np.array_equal(slots[:msg_len], claim))
                assert opens == (1 if msg_len < n else 0)                     # slot n - 1 is read by the full-length claim alone
                t_rows, claims, verdicts = np.concatenate([t_rows, extra[None]]), np.concatenate([claims, claim[None]]), verdicts + [opens]
            else:
                assert verdicts == [oracle.lwe_verify(Q_DEFAULT, n, k, SIGMA, KEY, r, c) for r, c in zip(t_rows, claims)]
            assert _verify_device(ctx, t_rows, claims) == verdicts, (kind, k, msg_len)
            # ---- 4. the host form ----
            assert pkg.verify_openings_words(ctx, t_rows, claims) == verdicts, (kind, k, msg_len, "host")
            if k == 3:
                assert [_opening_single(pkg, ctx, t_rows[j], claims[j]) for j in (0, 1, bad[0])] == [1, 0, -1]
            malformed[msg_len] = t_rows[[bad[0], 0, bad[1], bad[-1]]]           # a changed header, a fresh row, out-of-range words in u and in v
        # ---- 3. decode -------------------------------------------------------------------------------------------------------------
        rows = np.concatenate([fresh[5][1], fresh[n][1]])
        want_slots = np.concatenate([fresh[5][2][0], fresh[n][2][0]])
        want_bits = fresh[5][2][1] + fresh[n][2][1]
        for slots in (1, n):
            got, status, bits = _decode_device(ctx, rows, slots, True)
            assert status.tolist() == [1] * (2 * batch)
            assert np.array_equal(got, want_slots[:, :slots]), (kind, k, slots)
            assert bits.tolist() == want_bits, (kind, k, slots)               # exactly the model's, whatever `slots` is
            quiet, q_status, _ = _decode_device(ctx, rows, slots, False)
            assert np.array_equal(quiet, got) and q_status.tolist() == [1] * (2 * batch)
            host = ctx.decode_rows(rows, slots=slots, noise=True)
            assert np.array_equal(host[0], got) and host[1].tolist() == [1] * (2 * batch) and host[2].tolist() == want_bits
            host_quiet = ctx.decode_rows(rows, slots=slots)
            assert np.array_equal(host_quiet[0], got) and host_quiet[1].tolist() == [1] * (2 * batch)
        for msg_len in (5, n):
            fresh_slots, fresh_bits = fresh[msg_len][2][0][0], fresh[msg_len][2][1][0]
            for slots in (1, n):
                for noise in (True, False):
                    got, status, bits = _decode_device(ctx, malformed[msg_len], slots, noise)
                    assert status.tolist() == [-1, 1, -1, -1]
                    assert np.array_equal(got[1], fresh_slots[:slots]) and (not noise or bits[1] == fresh_bits)
                host = ctx.decode_rows(malformed[msg_len], slots=slots, noise=True)
                assert host[1].tolist() == [-1, 1, -1, -1] and np.array_equal(host[0][1], fresh_slots[:slots]) and host[2][1] == fresh_bits
    finally:
        ctx.close()


# ---- the fused pipeline at n = 2^16 and 2^17 ---------------------------------------------------------------------------------------------
def _large_rows(pkg, oracle, n, k, seed):
    q = oracle.L.oracle_lwe_select_modulus(0, n)
    ctx = _context(pkg, "default", n, k, q)
    assert ctx.pipeline == "fused" and ctx.commit_modulus == q
    rng = np.random.default_rng(seed)
    msgs = _messages(rng, ctx.plain_modulus, 2, 9)
    seeds = rng.integers(1, 2**63, size=2, dtype=np.uint64)
    return ctx, q, msgs, _device_rows(ctx, msgs, ctx.commit_keys(msgs, seeds))


@pytest.mark.parametrize("n,k", [(65536, 1), (65536, 3), (65536, 4), (131072, 3)])
def test_fused_decode_equals_the_model(pkg, oracle, n, k):
    """decode_top_inverse_kernel<R, NOISE> behind launch_mid_general<K, 1>: slots and the noise level of two fresh rows, exactly"""
    ctx, q, msgs, rows = _large_rows(pkg, oracle, n, k, n + k)
    try:
        want_slots, want_bits = _models(oracle, ctx, rows, msgs)
        got, status, bits = _decode_device(ctx, rows, n, True)
        assert status.tolist() == [1, 1] and np.array_equal(got, want_slots) and bits.tolist() == want_bits
        quiet, q_status, _ = _decode_device(ctx, rows, n, False)
        assert q_status.tolist() == [1, 1] and np.array_equal(quiet, got)
        few, _, few_bits = _decode_device(ctx, rows, 1, True)
        assert np.array_equal(few, want_slots[:, :1]) and few_bits.tolist() == want_bits
    finally:
        ctx.close()


@pytest.mark.parametrize("n,k", [(131072, 1), (131072, 3)])
def test_fused_openings_at_the_largest_degree(pkg, oracle, n, k):
    """two fresh rows open; a changed header, the modulus in the last word of the last u polynomial, and a wrong claim do not"""
    ctx, q, msgs, rows = _large_rows(pkg, oracle, n, k, n + 10 * k)
    try:
        t = ctx.plain_modulus
        embedded = msgs % np.uint64(t)
        assert _verify_device(ctx, rows, embedded) == [1, 1] == [oracle.lwe_verify(q, n, k, SIGMA, KEY, rows[j], embedded[j]) for j in range(2)]
        tampered, claims = rows[[0, 0, 1]].copy(), embedded[[0, 0, 1]].copy()
        tampered[0, 1] ^= 1                                                     # the magic
        tampered[1, 5 + (k - 1) * n + n - 1] = q
        claims[2, 8] = (int(claims[2, 8]) + 1) % t
        want = [-1, -1, 0]
        assert want == [oracle.lwe_verify(q, n, k, SIGMA, KEY, tampered[j], claims[j]) for j in range(3)]
        assert _verify_device(ctx, tampered, claims) == want
        assert pkg.verify_openings_words(ctx, tampered, claims) == want
    finally:
        ctx.close()
