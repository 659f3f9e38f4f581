"""GPU suite: batched prove_r1cs / prove_r1cs_zk (lsr_r1cs_prove_batch[_device]) against the one-by-one sequence of the reference —
oracle quotient, one Commitment per proof, Challenge::derive twice, eval_poly on the oracle's interpolants — and the batched
verifier and polynomial evaluation on the device (include/lambda_snark/prover.h)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prover_replay  # noqa: E402
from test_prover_gpu import extend_witness, random_r1cs  # noqa: E402

Q = 18446744069414584321
CQ = 17592186044417            # LweContext::modulus() of the profile below
M64 = (1 << 64) - 1
BLINDING = 12


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.LweContext(pkg.Params(q=CQ, n=4096, k=2, sigma=3.19), key_seed=0x5EED)
    yield c
    c.close()


def make_case(pkg, m, batch, free_vars=6, seed=0):
    rng = np.random.default_rng(seed + m)
    n, a, b, c = random_r1cs(rng, m, free_vars, fan_in=2)
    ws = np.stack([extend_witness(rng.integers(0, Q, size=free_vars, dtype=np.uint64), m, a, b) for _ in range(batch)])
    return rng, n, (a, b, c), ws


def one_by_one(pkg, oracle, ctx, m, mats, w, seed, n_public, r=None):
    """the reference's sequence for one witness: lib.rs:747-809 (r None) or 877-980"""
    ea, eb, ec = (oracle.sparse_mul_vec(mat, m, w, Q) for mat in mats)
    q_coeffs, ln = oracle.quotient(ea, eb, ec)
    assert ln >= 1
    quot = [int(v) for v in q_coeffs[:ln]]
    if r is not None:                                   # poly_add(Q, r Z_H), r1cs.rs:906-922
        quot = quot + [0] * (m + 1 - len(quot))
        quot[0] = (quot[0] - r) % Q
        quot[m] = (quot[m] + r) % Q
        while len(quot) > 1 and quot[-1] == 0:
            quot.pop()
    com = pkg.Commitment(ctx, np.array([v % CQ for v in quot], dtype=np.uint64), int(seed))
    row = com.as_words().copy()
    com.free()
    alpha, ha = prover_replay.challenge_derive([int(v) for v in w[:n_public]], row, Q)
    beta, hb = prover_replay.challenge_derive([alpha], row, Q)
    omega = oracle.prover_omega(m) if m > 1 else 1
    pa, pb, pc = ((oracle.cyclic_inverse(v, Q, omega) if m > 1 else np.array(v, dtype=np.uint64)) for v in (ea, eb, ec))
    qp = np.array(quot, dtype=np.uint64)
    ev = lambda p, x: int(oracle.eval_poly(p, x, Q))
    qa, qb = ev(qp, alpha), ev(qp, beta)
    proof = [alpha, beta, qa, qb, ev(pa, alpha), ev(pb, alpha), ev(pc, alpha), ev(pa, beta), ev(pb, beta), ev(pc, beta), qa, qb, r or 0]
    return row, proof, ha + hb, ln


@pytest.mark.parametrize("zk", [False, True])
@pytest.mark.parametrize("m", [1, 2, 64, 4096, 8192])
def test_prove_batch_matches_the_one_by_one_sequence(pkg, oracle, ctx, m, zk):
    batch, n_public = (3, 2) if m >= 4096 else (7, 3)
    rng, n, mats, ws = make_case(pkg, m, batch)
    seeds = np.arange(1, batch + 1, dtype=np.uint64) * np.uint64(104729)
    blind = rng.integers(0, 2**64, size=batch, dtype=np.uint64) if zk else None
    if zk:
        blind[0] = 0                                     # r = 0: Q' = Q
        blind[1] = np.uint64(Q + 5)                      # reduced mod p
    prover = pkg.R1csProver(m, n, *mats)
    rows, proofs, hashes, status = prover.prove_batch(ctx, ws, seeds, n_public, ctx.modulus(), blinding=blind)
    for i in range(batch):
        r = None if blind is None else int(blind[i]) % Q
        row, proof, h, ln = one_by_one(pkg, oracle, ctx, m, mats, ws[i], seeds[i], n_public, r)
        assert status[i] == ln
        assert np.array_equal(rows[i], row), i
        assert [int(v) for v in proofs[i]] == proof, i
        assert bytes(hashes[i]) == h
    assert list(pkg.verify_r1cs_batch(m, ws[:, :n_public], rows, proofs, zk=zk)) == [1] * batch
    prover.close()


def chained(pkg, lib, ctx, prover, ws, seeds, n_public):
    """rows, alphas, betas through the existing entry points (quotient -> commitment rows -> two transcripts)"""
    quot, lens = prover.quotient_batch(ws)
    rows = pkg.Commitment.batch_words(ctx, quot % np.uint64(CQ), seeds)
    batch, W = rows.shape
    publics = np.ascontiguousarray(ws[:, :n_public])
    alphas = np.zeros(batch, dtype=np.uint64); betas = np.zeros(batch, dtype=np.uint64)
    assert lib.lsr_fs_challenge_batch_flat(publics.ctypes.data, n_public, rows.ctypes.data, W, batch, Q, alphas.ctypes.data, None, 0) == 0
    assert lib.lsr_fs_challenge_batch_flat(alphas.ctypes.data, 1, rows.ctypes.data, W, batch, Q, betas.ctypes.data, None, 0) == 0
    return quot, lens, rows, alphas, betas


@pytest.mark.parametrize("m", [65536, 131072])
def test_large_m_matches_the_chained_entry_points(pkg, lib, oracle, ctx, m):
    batch, n_public = 4, 2
    rng, n, mats, ws = make_case(pkg, m, batch, free_vars=4)
    seeds = np.arange(11, 11 + batch, dtype=np.uint64)
    prover = pkg.R1csProver(m, n, *mats)
    rows, proofs, hashes, status = prover.prove_batch(ctx, ws, seeds, n_public, ctx.modulus())
    quot, lens, crows, alphas, betas = chained(pkg, lib, ctx, prover, ws, seeds, n_public)
    assert np.array_equal(status, lens) and np.array_equal(rows, crows)
    assert np.array_equal(proofs[:, 0], alphas) and np.array_equal(proofs[:, 1], betas)
    omega = oracle.prover_omega(m)
    for i in (0, 2, 3):                                  # O(m log m) oracle interpolation + eval_poly on picked instances
        ea, eb, ec = (oracle.sparse_mul_vec(mat, m, ws[i], Q) for mat in mats)
        pa, pb, pc = (oracle.cyclic_inverse(v, Q, omega) for v in (ea, eb, ec))
        a, b = int(alphas[i]), int(betas[i])
        ev = lambda p, x: int(oracle.eval_poly(p, x, Q))
        qa, qb = ev(quot[i, :lens[i]], a), ev(quot[i, :lens[i]], b)
        assert [int(v) for v in proofs[i]] == [a, b, qa, qb, ev(pa, a), ev(pb, a), ev(pc, a), ev(pa, b), ev(pb, b), ev(pc, b), qa, qb, 0]
    assert list(pkg.verify_r1cs_batch(m, ws[:, :n_public], rows, proofs)) == [1] * batch
    prover.close()


def test_unsatisfied_witness_gets_status_zero(pkg, oracle, ctx):
    m, batch, n_public = 64, 5, 2
    rng, n, mats, ws = make_case(pkg, m, batch)
    ws[2, n - 3] = np.uint64((int(ws[2, n - 3]) + 1) % Q)
    seeds = np.arange(1, batch + 1, dtype=np.uint64)
    prover = pkg.R1csProver(m, n, *mats)
    rows, proofs, hashes, status = prover.prove_batch(ctx, ws, seeds, n_public, ctx.modulus())
    assert status[2] == 0
    for i in (0, 1, 3, 4):
        row, proof, h, ln = one_by_one(pkg, oracle, ctx, m, mats, ws[i], seeds[i], n_public)
        assert status[i] == ln and np.array_equal(rows[i], row) and [int(v) for v in proofs[i]] == proof and bytes(hashes[i]) == h
    prover.close()


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


@pytest.mark.parametrize("zk", [False, True])
def test_device_variant_equals_host_and_multi_chunk(pkg, ctx, zk, monkeypatch):
    import torch
    m, batch, n_public = 256, 37, 3
    rng, n, mats, ws = make_case(pkg, m, batch)
    seeds = rng.integers(1, 2**63, size=batch, dtype=np.uint64)
    blind = rng.integers(0, 2**64, size=batch, dtype=np.uint64) if zk else None
    prover = pkg.R1csProver(m, n, *mats)
    rows, proofs, hashes, status = prover.prove_batch(ctx, ws, seeds, n_public, ctx.modulus(), blinding=blind)
    W = ctx.commitment_words
    dw = to_dev(torch, ws)
    db = to_dev(torch, blind) if zk else None
    drows = torch.zeros((batch, W), dtype=torch.int64, device="cuda")
    dproofs = torch.zeros((batch, 13), dtype=torch.int64, device="cuda")
    dhash = torch.zeros((batch, 64), dtype=torch.uint8, device="cuda")
    dstat = torch.zeros(batch, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream()
    prover.prove_batch_device(ctx, dw.data_ptr(), batch, seeds, n_public, ctx.modulus(), drows.data_ptr(), dproofs.data_ptr(), dhash.data_ptr(),
                              dstat.data_ptr(), None if db is None else db.data_ptr(), s.cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(drows.cpu().numpy().view(np.uint64), rows)
    assert np.array_equal(dproofs.cpu().numpy().view(np.uint64), proofs)
    assert np.array_equal(dhash.cpu().numpy(), hashes.reshape(batch, 64))
    assert np.array_equal(dstat.cpu().numpy().view(np.uint32), status)
    # a plan forced into chunks of 8 instances (2^11 evaluations per pass) gives the same words
    monkeypatch.setenv("LAMBDA_SNARK_QUOTIENT_CHUNK_LOG2", "11")
    small = pkg.R1csProver(m, n, *mats)
    monkeypatch.delenv("LAMBDA_SNARK_QUOTIENT_CHUNK_LOG2")
    r2, p2, h2, s2 = small.prove_batch(ctx, ws, seeds, n_public, ctx.modulus(), blinding=blind)
    assert np.array_equal(r2, rows) and np.array_equal(p2, proofs) and np.array_equal(h2, hashes) and np.array_equal(s2, status)
    small.close(); prover.close()


def test_two_streams_two_provers_and_refusals(pkg, ctx):
    import torch
    m, batch, n_public = 128, 16, 2
    rng, n, mats, ws = make_case(pkg, m, batch)
    seeds = np.arange(3, 3 + batch, dtype=np.uint64)
    provers = [pkg.R1csProver(m, n, *mats) for _ in range(2)]
    ref = provers[0].prove_batch(ctx, ws, seeds, n_public, ctx.modulus())
    ctx2 = pkg.LweContext(pkg.Params(q=CQ, n=4096, k=2, sigma=3.19), key_seed=0x5EED)
    W = ctx.commitment_words
    dw = to_dev(torch, ws)
    outs, streams = [], [torch.cuda.Stream(), torch.cuda.Stream()]
    for k in range(2):
        outs.append((torch.zeros((batch, W), dtype=torch.int64, device="cuda"), torch.zeros((batch, 13), dtype=torch.int64, device="cuda"),
                     torch.zeros(batch, dtype=torch.int32, device="cuda")))
    torch.cuda.synchronize()
    for k in range(2):
        c = ctx if k == 0 else ctx2
        provers[k].prove_batch_device(c, dw.data_ptr(), batch, seeds, n_public, c.modulus(), outs[k][0].data_ptr(), outs[k][1].data_ptr(), 0,
                                      outs[k][2].data_ptr(), None, streams[k].cuda_stream)
    torch.cuda.synchronize()
    for k in range(2):
        assert np.array_equal(outs[k][0].cpu().numpy().view(np.uint64), ref[0])
        assert np.array_equal(outs[k][1].cpu().numpy().view(np.uint64), ref[1])
    # seed 0 is refused on the device; the host call turns it into fresh entropy whose proof verifies
    zs = seeds.copy(); zs[5] = 0
    with pytest.raises(pkg.CoreError, match="seed 0"):
        provers[0].prove_batch_device(ctx, dw.data_ptr(), batch, zs, n_public, ctx.modulus(), outs[0][0].data_ptr(), outs[0][1].data_ptr(), 0,
                                      outs[0][2].data_ptr(), None, 0)
    rows, proofs, _, status = provers[0].prove_batch(ctx, ws, zs, n_public, ctx.modulus())
    assert (status >= 1).all() and list(pkg.verify_r1cs_batch(m, ws[:, :n_public], rows, proofs)) == [1] * batch
    assert np.array_equal(np.delete(rows, 5, 0), np.delete(ref[0], 5, 0))
    # refused under stream capture
    g, cs = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(cs):
        with torch.cuda.graph(g, stream=cs):
            with pytest.raises(pkg.CoreError, match="capturable"):
                provers[1].prove_batch_device(ctx2, dw.data_ptr(), batch, seeds, n_public, ctx2.modulus(), outs[1][0].data_ptr(),
                                              outs[1][1].data_ptr(), 0, outs[1][2].data_ptr(), None, cs.cuda_stream)
    for p in provers:
        p.close()
    ctx2.close()


def test_eval_batch_device_matches_eval_poly(pkg, oracle):
    import torch
    rng = np.random.default_rng(5)
    omega = oracle.prover_omega(1 << 10)
    special = [0, 1, Q - 1, Q, M64, pow(omega, 3, Q), pow(omega, 1023, Q)]
    for length in (1, 7, 255, 257, 1001, 4096, 300001):
        batch, ppp = 3, len(special) + 2
        coeffs = rng.integers(0, 2**64, size=(batch, length), dtype=np.uint64)
        coeffs[0, :3] = [Q - 1, Q, M64][:min(3, length)]
        coeffs[1, -1] = np.uint64(M64)
        pts = np.array([special + [int(rng.integers(0, 2**64, dtype=np.uint64)) for _ in range(2)] for _ in range(batch)], dtype=np.uint64)
        out = torch.zeros((batch, ppp), dtype=torch.int64, device="cuda")
        dc, dp = to_dev(torch, coeffs), to_dev(torch, pts)
        pkg.prover_eval_batch_device(dc.data_ptr(), length, batch, dp.data_ptr(), ppp, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint64)
        for i in range(batch):
            red = np.array([int(c) % Q for c in coeffs[i]], dtype=np.uint64)
            for k in range(ppp):
                assert int(got[i, k]) == int(oracle.eval_poly(red, int(pts[i, k]) % Q, Q)), (length, i, k)


@pytest.mark.parametrize("zk", [False, True])
def test_verify_device_equals_host_on_the_tamper_matrix(pkg, ctx, zk):
    import torch
    m, batch, n_public = 64, 6, 2
    rng, n, mats, ws = make_case(pkg, m, batch)
    prover = pkg.R1csProver(m, n, *mats)
    blind = rng.integers(0, 2**64, size=batch, dtype=np.uint64) if zk else None
    rows, proofs, _, _ = prover.prove_batch(ctx, ws, np.arange(1, batch + 1, dtype=np.uint64), n_public, ctx.modulus(), blinding=blind)
    cases = [(rows, proofs, ws[:, :n_public].copy())]
    for w in range(13):
        for val in (None, Q, M64):
            p = proofs.copy()
            p[w % batch, w] = np.uint64(val) if val is not None else p[w % batch, w] ^ np.uint64(2)
            cases.append((rows, p, ws[:, :n_public].copy()))
    r2 = rows.copy(); r2[1, 7] ^= np.uint64(1); cases.append((r2, proofs, ws[:, :n_public].copy()))
    pb = ws[:, :n_public].copy(); pb[4, 1] ^= np.uint64(1); cases.append((rows, proofs, pb))
    for rr, pp, pub in cases:
        host = pkg.verify_r1cs_batch(m, pub, rr, pp, zk=zk)
        dres = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
        dpub, drows, dpr = to_dev(torch, pub), to_dev(torch, rr), to_dev(torch, pp)
        pkg.verify_r1cs_batch_device(m, dpub.data_ptr(), n_public, drows.data_ptr(), rr.shape[1], dpr.data_ptr(), batch, dres.data_ptr(), zk=zk,
                                     stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert list(dres.cpu().numpy()) == list(host)
    assert list(pkg.verify_r1cs_batch(m, ws[:, :n_public], rows, proofs, zk=zk)) == [1] * batch
    prover.close()


def test_bench_shaped_batch(pkg, lib, oracle, ctx):
    """m = 4096, 4096 proofs (n = 4096, k = 2): the chain's rows and challenges, sampled oracle evaluations, all proofs verify"""
    m, batch, n_public, free_vars = 4096, 4096, 2, 4
    rng = np.random.default_rng(4096)
    n, a, b, c = random_r1cs(rng, m, free_vars, fan_in=2)
    base = extend_witness(rng.integers(0, Q, size=free_vars, dtype=np.uint64), m, a, b)
    ws = np.stack([base] * batch)
    ws[:, :free_vars] = rng.integers(0, Q, size=(batch, free_vars), dtype=np.uint64)
    picks = (0, 1234, 4095)
    for i in picks:
        ws[i] = extend_witness(ws[i, :free_vars], m, a, b)
    prover = pkg.R1csProver(m, n, a, b, c)
    seeds = np.arange(1, batch + 1, dtype=np.uint64)
    rows, proofs, hashes, status = prover.prove_batch(ctx, ws, seeds, n_public, ctx.modulus())
    quot, lens, crows, alphas, betas = chained(pkg, lib, ctx, prover, ws, seeds, n_public)
    assert np.array_equal(status, lens) and np.array_equal(rows, crows)
    assert np.array_equal(proofs[:, 0], alphas) and np.array_equal(proofs[:, 1], betas)
    for i in picks:
        row, proof, h, ln = one_by_one(pkg, oracle, ctx, m, (a, b, c), ws[i], seeds[i], n_public)
        assert status[i] == ln and [int(v) for v in proofs[i]] == proof and bytes(hashes[i]) == h
    ok = status > 0
    assert ok[list(picks)].all()
    assert (pkg.verify_r1cs_batch(m, ws[:, :n_public], rows, proofs)[ok] == 1).all()
    prover.close()
