"""GPU suite: the Lagrange (baseline) path of lsr_r1cs_prove_batch[_device] and lsr_r1cs_verify_batch_mod[_device]
against the one-by-one sequence of the reference — quotient, one Commitment per proof, Challenge::derive twice, eval_poly — restated
by tests/lagrange_oracle.py."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lagrange_oracle as lo  # noqa: E402

GOLD = 18446744069414584321
CQ = 17592186044417
P44 = (1 << 44) + 1
MODULI = [P44, (1 << 31) - 1, 17592186044423, 97, GOLD]
MS = [1, 2, 3, 5, 10, 16, 17, 30, 100]


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.LweContext(pkg.Params(q=CQ, n=4096, k=2, sigma=3.19), key_seed=0x5EED)
    yield c
    c.close()


def commit_fn(pkg, ctx):
    def commit(msg, seed):
        com = pkg.Commitment(ctx, np.array([v % CQ for v in msg], dtype=np.uint64), int(seed))
        words = com.as_words().copy()
        com.free()
        return words
    return commit


def allowed(m, q):
    if lo.uses_ntt(m, q):
        return False
    try:
        lo.domain(m, q)
        return not (q == P44 and m >= 18) and not (q == 97 and m > 97)
    except lo.NotAUnit:
        return False


def make_case(m, q, batch, free_vars=4, seed=0):
    rng = np.random.default_rng(seed + m + q % 997)
    n, a, b, c = lo.random_circuit(rng, m, free_vars, q)
    ws = np.stack([lo.extend_witness(rng.integers(0, 2**64, size=free_vars, dtype=np.uint64), m, a, b, q) for _ in range(batch)])
    return rng, n, (a, b, c), ws


CASES = [(m, q) for q in MODULI for m in MS if allowed(m, q)]


@pytest.mark.parametrize("zk", [False, True])
@pytest.mark.parametrize("m,q", CASES)
def test_prove_batch_is_bit_exact(pkg, ctx, m, q, zk):
    batch, n_public = 4, 2
    rng, n, mats, ws = make_case(m, q, batch)
    seeds = np.arange(1, batch + 1, dtype=np.uint64) * np.uint64(7919)
    blind = rng.integers(0, 2**64, size=batch, dtype=np.uint64) if zk else None
    if zk:
        blind[0] = 0
        blind[1] = np.uint64(q + 3 if q + 3 < 2**64 else q)         # r >= q is reduced
    prover = pkg.R1csProver(m, n, *mats, modulus=q)
    assert not prover.uses_ntt and prover.modulus == q
    rows, proofs, hashes, status = prover.prove_batch(ctx, ws, seeds, n_public, ctx.modulus(), blinding=blind)
    quot, lens = prover.quotient_batch(ws)
    rows_l = lo.interpolation_rows(m, q)
    for i in range(batch):
        r = None if blind is None else int(blind[i])
        row, proof, h, ln = lo.prove_one(mats, m, q, ws[i], n_public, commit_fn(pkg, ctx), seeds[i], r, rows_l)
        assert status[i] == ln == lens[i]
        assert np.array_equal(rows[i], row), i
        assert [int(v) for v in proofs[i]] == proof, i
        assert bytes(hashes[i]) == h
    assert list(pkg.verify_r1cs_batch(m, ws[:, :n_public], rows, proofs, zk=zk, modulus=q)) == [1] * batch
    prover.close()


def test_non_unit_domain_is_refused(pkg):
    rng, n, mats, ws = make_case(18, P44, 1)
    with pytest.raises(pkg.CoreError, match="not a unit"):
        pkg.R1csProver(18, n, *mats, modulus=P44)
    with pytest.raises(pkg.CoreError, match="odd"):
        pkg.R1csProver(4, 10, [(0, 0, 1)], [(0, 0, 1)], [(0, 0, 1)], modulus=1 << 44)


@pytest.mark.parametrize("m", [4, 8, 6])
def test_the_omega_domain_quirk(pkg, ctx, m):
    q = lo.QUIRK_MODULUS
    rng, n, mats, ws = make_case(m, q, 3)
    ws[2] = 0                                                         # all-zero evaluations: N = 0 proves
    seeds = np.array([3, 4, 5], dtype=np.uint64)
    prover = pkg.R1csProver(m, n, *mats, modulus=q)
    rows, proofs, hashes, status = prover.prove_batch(ctx, ws, seeds, 2, ctx.modulus())
    for i in range(3):
        want = lo.prove_one(mats, m, q, ws[i], 2, commit_fn(pkg, ctx), seeds[i])
        if want is None:
            assert status[i] == 0
        else:
            row, proof, h, ln = want
            assert status[i] == ln and np.array_equal(rows[i], row) and [int(v) for v in proofs[i]] == proof
    if m in (4, 8):     # satisfying witnesses with non-zero evaluations leave a remainder on {omega^j}
        assert list(status) == [0, 0, 1]
    else:
        assert (status >= 1).all()
    prover.close()


def test_m1024_matches_the_oracle(pkg, ctx):
    m, q, batch = 1024, 17592186044423, 3
    rng, n, mats, ws = make_case(m, q, batch)
    prover = pkg.R1csProver(m, n, *mats, modulus=q)
    seeds = np.array([11, 12, 13], dtype=np.uint64)
    rows, proofs, hashes, status = prover.prove_batch(ctx, ws, seeds, 2, ctx.modulus())
    rows_l = lo.interpolation_rows(m, q)
    for i in (0, 2):
        row, proof, h, ln = lo.prove_one(mats, m, q, ws[i], 2, commit_fn(pkg, ctx), seeds[i], None, rows_l)
        assert status[i] == ln and np.array_equal(rows[i], row) and [int(v) for v in proofs[i]] == proof and bytes(hashes[i]) == h
    prover.close()


def test_m8192_interpolants_quotient_and_verifiers(pkg, ctx):
    import torch
    m, q, batch = 8192, 17592186044423, 2
    rng, n, mats, ws = make_case(m, q, batch, free_vars=3)
    prover = pkg.R1csProver(m, n, *mats, modulus=q)
    rows, proofs, _, status = prover.prove_batch(ctx, ws, np.array([1, 2], dtype=np.uint64), 2, ctx.modulus())
    assert (status >= 1).all()
    assert list(pkg.verify_r1cs_batch(m, ws[:, :2], rows, proofs, modulus=q)) == [1, 1]
    dres = torch.zeros(batch, dtype=torch.int32, device="cuda")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
    dp, dr, dpr = t(ws[:, :2]), t(rows), t(proofs)
    pkg.verify_r1cs_batch_device(m, dp.data_ptr(), 2, dr.data_ptr(), rows.shape[1], dpr.data_ptr(), batch, dres.data_ptr(), modulus=q,
                                 stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert list(dres.cpu().numpy()) == [1, 1]
    ea, eb, ec = prover.compute_constraint_evals(ws)
    pa, pb, pc = prover.interpolate_batch(ws)
    quot, lens = prover.quotient_batch(ws)
    for i in range(batch):
        for x in [0, 1, 4095, 8191] + [int(v) for v in rng.integers(0, m, size=4)]:
            assert lo.eval_poly(pa[i], x, q) == int(ea[i, x]) and lo.eval_poly(pc[i], x, q) == int(ec[i, x])
        for _ in range(3):
            x = int(rng.integers(0, q))
            nval = (lo.eval_poly(pa[i], x, q) * lo.eval_poly(pb[i], x, q) - lo.eval_poly(pc[i], x, q)) % q
            assert nval == lo.eval_poly(quot[i, :lens[i]], x, q) * lo.eval_vanishing(m, x, q) % q
    prover.close()


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


@pytest.mark.parametrize("zk", [False, True])
def test_unsatisfied_device_host_chunking(pkg, ctx, zk, monkeypatch):
    import torch
    m, q, batch, n_public = 30, (1 << 31) - 1, 21, 3
    rng, n, mats, ws = make_case(m, q, batch)
    ws[4, n - 2] = np.uint64((int(ws[4, n - 2]) + 1) % q)
    seeds = rng.integers(1, 2**63, size=batch, dtype=np.uint64)
    blind = rng.integers(0, 2**64, size=batch, dtype=np.uint64) if zk else None
    prover = pkg.R1csProver(m, n, *mats, modulus=q)
    rows, proofs, hashes, status = prover.prove_batch(ctx, ws, seeds, n_public, ctx.modulus(), blinding=blind)
    assert status[4] == 0 and (np.delete(status, 4) >= 1).all()
    W = ctx.commitment_words
    dw = to_dev(torch, ws)
    db = to_dev(torch, blind) if zk else None
    drows = torch.zeros((batch, W), dtype=torch.int64, device="cuda")
    dproofs = torch.zeros((batch, 13), dtype=torch.int64, device="cuda")
    dhash = torch.zeros((batch, 64), dtype=torch.uint8, device="cuda")
    dstat = torch.zeros(batch, dtype=torch.int32, device="cuda")
    prover.prove_batch_device(ctx, dw.data_ptr(), batch, seeds, n_public, ctx.modulus(), drows.data_ptr(), dproofs.data_ptr(), dhash.data_ptr(),
                              dstat.data_ptr(), None if db is None else db.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ok = status > 0
    assert np.array_equal(dstat.cpu().numpy().view(np.uint32), status)
    assert np.array_equal(drows.cpu().numpy().view(np.uint64)[ok], rows[ok])
    assert np.array_equal(dproofs.cpu().numpy().view(np.uint64)[ok], proofs[ok])
    assert np.array_equal(dhash.cpu().numpy()[ok], hashes.reshape(batch, 64)[ok])
    monkeypatch.setenv("LAMBDA_SNARK_QUOTIENT_CHUNK_LOG2", "8")          # 256 / 30 = 8 instances per pass
    small = pkg.R1csProver(m, n, *mats, modulus=q)
    monkeypatch.delenv("LAMBDA_SNARK_QUOTIENT_CHUNK_LOG2")
    r2, p2, h2, s2 = small.prove_batch(ctx, ws, seeds, n_public, ctx.modulus(), blinding=blind)
    assert np.array_equal(s2, status) and np.array_equal(r2[ok], rows[ok]) and np.array_equal(p2[ok], proofs[ok]) and np.array_equal(h2[ok], hashes[ok])
    assert list(pkg.verify_r1cs_batch(m, ws[:, :n_public], rows, proofs, zk=zk, modulus=q)[ok]) == [1] * int(ok.sum())
    small.close(); prover.close()


def test_two_streams_capture_and_seed_zero(pkg, ctx):
    import torch
    m, q, batch, n_public = 10, 17592186044423, 16, 2
    rng, n, mats, ws = make_case(m, q, batch)
    seeds = np.arange(3, 3 + batch, dtype=np.uint64)
    provers = [pkg.R1csProver(m, n, *mats, modulus=q) for _ in range(2)]
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
    zs = seeds.copy(); zs[5] = 0
    with pytest.raises(pkg.CoreError, match="seed 0"):
        provers[0].prove_batch_device(ctx, dw.data_ptr(), batch, zs, n_public, ctx.modulus(), outs[0][0].data_ptr(), outs[0][1].data_ptr(), 0,
                                      outs[0][2].data_ptr(), None, 0)
    rows, proofs, _, status = provers[0].prove_batch(ctx, ws, zs, n_public, ctx.modulus())
    assert (status >= 1).all() and list(pkg.verify_r1cs_batch(m, ws[:, :n_public], rows, proofs, modulus=q)) == [1] * batch
    assert np.array_equal(np.delete(rows, 5, 0), np.delete(ref[0], 5, 0))
    g, cs = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(cs):
        with torch.cuda.graph(g, stream=cs):
            with pytest.raises(pkg.CoreError, match="capturable"):
                provers[1].prove_batch_device(ctx2, dw.data_ptr(), batch, seeds, n_public, ctx2.modulus(), outs[1][0].data_ptr(),
                                              outs[1][1].data_ptr(), 0, outs[1][2].data_ptr(), None, cs.cuda_stream)
    for p in provers:
        p.close()
    ctx2.close()


@pytest.mark.parametrize("m", [16, 64])
def test_create_mod_on_the_ntt_path_equals_create(pkg, ctx, m):
    rng, n, mats, ws = make_case(m, GOLD, 3)
    a = pkg.R1csProver(m, n, *mats)
    b = pkg.R1csProver(m, n, *mats, modulus=GOLD)
    assert b.uses_ntt and a.uses_ntt
    seeds = np.array([1, 2, 3], dtype=np.uint64)
    ra = a.prove_batch(ctx, ws, seeds, 2, ctx.modulus())
    rb = b.prove_batch(ctx, ws, seeds, 2, ctx.modulus())
    for x, y in zip(ra, rb):
        assert np.array_equal(x, y)
    a.close(); b.close()


@pytest.mark.parametrize("zk", [False, True])
def test_verify_mod_device_equals_host_on_the_tamper_matrix(pkg, ctx, zk):
    import torch
    m, q, batch, n_public = 17, 17592186044423, 6, 2
    rng, n, mats, ws = make_case(m, q, batch)
    prover = pkg.R1csProver(m, n, *mats, modulus=q)
    blind = rng.integers(0, 2**64, size=batch, dtype=np.uint64) if zk else None
    rows, proofs, _, _ = prover.prove_batch(ctx, ws, np.arange(1, batch + 1, dtype=np.uint64), n_public, ctx.modulus(), blinding=blind)
    cases = [(rows, proofs, ws[:, :n_public].copy())]
    for w in range(13):
        for val in (None, q, 2**64 - 1):
            p = proofs.copy()
            p[w % batch, w] = np.uint64(val) if val is not None else p[w % batch, w] ^ np.uint64(2)
            cases.append((rows, p, ws[:, :n_public].copy()))
    r2 = rows.copy(); r2[1, 7] ^= np.uint64(1); cases.append((r2, proofs, ws[:, :n_public].copy()))
    for rr, pp, pub in cases:
        host = pkg.verify_r1cs_batch(m, pub, rr, pp, zk=zk, modulus=q)
        dres = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
        dpub, drows, dpr = to_dev(torch, pub), to_dev(torch, rr), to_dev(torch, pp)
        pkg.verify_r1cs_batch_device(m, dpub.data_ptr(), n_public, drows.data_ptr(), rr.shape[1], dpr.data_ptr(), batch, dres.data_ptr(), zk=zk,
                                     stream=torch.cuda.current_stream().cuda_stream, modulus=q)
        torch.cuda.synchronize()
        assert list(dres.cpu().numpy()) == list(host)
    assert list(pkg.verify_r1cs_batch(m, ws[:, :n_public], rows, proofs, zk=zk, modulus=q)) == [1] * batch
    prover.close()
