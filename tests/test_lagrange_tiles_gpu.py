"""GPU suite: the Lagrange (baseline) prove path (lsr_lagrange.hip, lsr_lagrange_kernels.hpp, lsr_montq.hpp) past one
row tile, at the switch between its two interpolation kernels and at moduli up to 2^64 - 59.  tests/test_r1cs_lagrange_gpu.py never
launches a second 64-row tile (at most 63 rows), runs no m between 30 and 100, one modulus above 2^63 (Goldilocks, whose Montgomery
constants are special) and random, reduced data only.

Every comparison is exact, with tests/lagrange_oracle.py (O(m^2), Python integers) or, at m = 8192, with polynomial identities at
fixed points through tests/lagrange_directed.py's O(m) `interpolant_at`, which shares nothing with any interpolation matrix.

Shapes: rows = 3 batch of the [3][batch][m] evaluation buffer in tiles of 64.  batch 22 -> 66 rows (two tiles, the second two rows
long, the boundary inside C); batch 43 -> 129 rows (three tiles, the last one row long, boundaries inside B and inside C).  m = 63,
64 run the small kernel (m = 64 fills both LDS arrays), m = 65 the tiled one with a second column tile one column wide and a K block
of one; m = 127, 128, 129 the same one tile further, and lag_eval_kernel's 64-lane stride over m and m + 1 words on either side.

`carry_instance` (m = 64, 65 at 2^64 - 59) is the one input on this path whose 192-bit sum leaves acc_reduce with a carry out of 64
bits: random data reaches that branch with probability about 2^-51 per sum."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lagrange_directed as ld  # noqa: E402
import lagrange_oracle as lo  # noqa: E402
from lagrange_directed import (Q63, Q64, QC, test_carry_instance_sum_and_quotient,  # noqa: E402,F401 (collected here: CPU tests)
                               test_interpolant_at_equals_the_oracle, test_selector_circuit_reproduces_its_vectors,
                               test_steered_is_all_q_minus_one_and_satisfied)

CQ = 17592186044417
N_PUBLIC = 2
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.LweContext(pkg.Params(q=CQ, n=4096, k=2, sigma=3.19), key_seed=0x5EED)
    yield c
    c.close()


@pytest.fixture
def open_prover(pkg):
    """R1csProver(m, n, mats, q), closed when the test ends however it ends: a failing case must not leave its stream and workspace to
    the garbage collector while later cases run"""
    opened = []

    def make(m, n, mats, q):
        prover = pkg.R1csProver(m, n, *mats, modulus=q)
        opened.append(prover)
        assert not prover.uses_ntt and prover.modulus == q
        return prover
    yield make
    for prover in opened:
        prover.close()


def commit_fn(pkg, ctx):
    def commit(msg, seed):
        com = pkg.Commitment(ctx, np.array([v % CQ for v in msg], dtype=np.uint64), int(seed))
        words = com.as_words().copy()
        com.free()
        return words
    return commit


def ints(a):
    return [int(v) for v in a]


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


@functools.lru_cache(maxsize=None)
def random_case(m, q, batch):
    """A random circuit with `batch` satisfying witnesses and the oracle's evaluations, interpolants and quotients (computed once,
    shared by the tests that use the same shape, never written to)."""
    rng = np.random.default_rng(1000 * m + batch + q % 997)
    n, a, b, c = lo.random_circuit(rng, m, 4, q)
    ws = np.stack([lo.extend_witness(rng.integers(0, 2**64, size=4, dtype=np.uint64), m, a, b, q) for _ in range(batch)])
    ws.setflags(write=False)
    rows_l = lo.interpolation_rows(m, q)
    evals = [[lo.mat_vec(e, m, w, q) for e in (a, b, c)] for w in ws]
    flat = lo.interpolate_many([v for e in evals for v in e], q, rows_l)
    coefs = [flat[3 * i:3 * i + 3] for i in range(batch)]
    quots = [lo.quotient(e, q, rows_l) for e in evals]
    assert all(qq is not None for qq in quots)
    return n, (a, b, c), ws, rows_l, evals, coefs, quots


def boundary_instances(batch):
    """instance 0, the instances whose rows lie on both sides of each 64-row boundary of the [3][batch][m] buffer, and the last"""
    picks = {0, batch - 1}
    for r in range(64, 3 * batch, 64):
        picks |= {(r - 1) % batch, r % batch}
    return sorted(picks)


def check_stages(prover, ws, evals, coefs, quots, skip=()):
    """compute_constraint_evals, interpolate_batch and quotient_batch against the oracle, every instance not in `skip`"""
    got_e = prover.compute_constraint_evals(ws)
    got_c = prover.interpolate_batch(ws)
    quot, lens = prover.quotient_batch(ws)
    for i in range(len(ws)):
        for k in range(3):
            assert ints(got_e[k][i]) == evals[i][k], ("evals", i, k)
            assert ints(got_c[k][i]) == coefs[i][k], ("interpolant", i, k)
        if i in skip:
            continue
        assert lens[i] == len(quots[i]), ("length", i)
        assert ints(quot[i, :lens[i]]) == quots[i], ("quotient", i)
        assert not quot[i, lens[i]:].any()
    return quot, lens


def check_proofs(pkg, ctx, prover, mats, m, q, ws, rows_l, picks, seeds, blind, bad=()):
    rows, proofs, hashes, status = prover.prove_batch(ctx, ws, seeds, N_PUBLIC, ctx.modulus(), blinding=blind)
    for i in picks:
        r = None if blind is None else int(blind[i])
        want = lo.prove_one(mats, m, q, ws[i], N_PUBLIC, commit_fn(pkg, ctx), seeds[i], r, rows_l)
        if i in bad:
            assert want is None and status[i] == 0
            continue
        row, proof, h, ln = want
        assert status[i] == ln, i
        assert np.array_equal(rows[i], row), i
        assert ints(proofs[i]) == proof, i
        assert bytes(hashes[i]) == h, i
    ok = np.array([i not in bad for i in range(len(ws))])
    assert list(status[~ok]) == [0] * len(bad) and (status[ok] >= 1).all()
    assert list(pkg.verify_r1cs_batch(m, ws[ok][:, :N_PUBLIC], rows[ok], proofs[ok], zk=blind is not None, modulus=q)) == [1] * int(ok.sum())
    return rows, proofs, hashes, status


def blinding_words(q, batch, seed):
    blind = np.random.default_rng(seed).integers(0, 2**64, size=batch, dtype=np.uint64)
    blind[0] = 0
    blind[batch - 1] = np.uint64(M64)                                # r >= q is reduced
    return blind


# ---- a. row tiles and the kernel switch -------------------------------------------------------------------------------------
TILE_CASES = ([(m, Q64, batch) for m in (63, 64, 65, 127, 128, 129) for batch in (22, 43)]
              + [(m, q, 43) for q in (QC, Q63, 32749, 16411) for m in (64, 65)])


@pytest.mark.gpu
@pytest.mark.parametrize("m,q,batch", TILE_CASES)
def test_row_tiles_and_the_kernel_switch(pkg, ctx, open_prover, m, q, batch):
    n, mats, ws, rows_l, evals, coefs, quots = random_case(m, q, batch)
    assert 3 * batch > 64 and (3 * batch) % 64 != 0
    prover = open_prover(m, n, mats, q)
    check_stages(prover, ws, evals, coefs, quots)
    seeds = np.arange(1, batch + 1, dtype=np.uint64) * np.uint64(7919)
    picks = boundary_instances(batch)
    assert picks == ([0, 19, 20, 21] if batch == 22 else [0, 20, 21, 41, 42])
    for blind in (None, blinding_words(q, batch, m)):
        check_proofs(pkg, ctx, prover, mats, m, q, ws, rows_l, picks, seeds, blind)


@pytest.mark.gpu
def test_chunked_passes_of_93_and_36_rows_equal_one_pass(pkg, ctx, open_prover, monkeypatch):
    m, q, batch = 65, Q64, 43
    n, mats, ws, rows_l, evals, coefs, quots = random_case(m, q, batch)
    seeds = np.arange(1, batch + 1, dtype=np.uint64) * np.uint64(104729)
    blind = blinding_words(q, batch, 7)
    whole = open_prover(m, n, mats, q)
    monkeypatch.setenv("LAMBDA_SNARK_QUOTIENT_CHUNK_LOG2", "11")          # 2048 / 65 = 31 instances = 93 rows per pass, then 12
    small = open_prover(m, n, mats, q)
    monkeypatch.delenv("LAMBDA_SNARK_QUOTIENT_CHUNK_LOG2")
    check_stages(small, ws, evals, coefs, quots)
    for b in (None, blind):
        want = whole.prove_batch(ctx, ws, seeds, N_PUBLIC, ctx.modulus(), blinding=b)
        got = small.prove_batch(ctx, ws, seeds, N_PUBLIC, ctx.modulus(), blinding=b)
        assert (want[3] >= 1).all()
        for x, y in zip(want, got):
            assert np.array_equal(x, y)
    check_proofs(pkg, ctx, small, mats, m, q, ws, rows_l, [0, 30, 31, 42], seeds, blind)


# ---- b. unsatisfied instances in a later tile -------------------------------------------------------------------------------
@pytest.mark.gpu
def test_unsatisfied_instances_in_later_tiles(pkg, ctx, open_prover):
    m, q, batch, bad = 64, Q64, 43, (21, 22, 42)
    n, mats, ws0, rows_l, evals0, coefs0, quots = random_case(m, q, batch)
    ws = ws0.copy()
    evals, coefs = [list(e) for e in evals0], [list(c) for c in coefs0]
    for i in bad:                                                        # the last constraint's output: C z changes, A z and B z do not
        ws[i, n - 1] = np.uint64((int(ws[i, n - 1]) + 1) % q)
        evals[i][2] = lo.mat_vec(mats[2], m, ws[i], q)
        coefs[i][2] = lo.interpolate(evals[i][2], q)
    prover = open_prover(m, n, mats, q)
    quot, lens = check_stages(prover, ws, evals, coefs, quots, skip=bad)
    assert [i for i in range(batch) if lens[i] == 0] == list(bad)
    seeds = np.arange(1, batch + 1, dtype=np.uint64) * np.uint64(31337)
    picks = sorted(set(boundary_instances(batch)) | {20, 21, 22, 23, 41, 42})
    for blind in (None, blinding_words(q, batch, 3)):
        check_proofs(pkg, ctx, prover, mats, m, q, ws, rows_l, picks, seeds, blind, bad=bad)


# ---- c. unreduced witness words ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("q", [97, 32749])
def test_unreduced_witness_words(pkg, ctx, open_prover, q):
    m, batch = 30, 4
    n, mats, ws0, rows_l, evals, coefs, quots = random_case(m, q, batch)
    rng = np.random.default_rng(q)
    ws = ws0.copy()
    for i in range(batch):
        for j in range(n):
            if j < N_PUBLIC or rng.integers(0, 3):                       # the public words always, two in three of the others
                w = int(ws[i, j])
                ws[i, j] = np.uint64(w + int(rng.integers(0, (M64 - w) // q + 1)) * q)
        j = N_PUBLIC + i                                                 # one word per instance as high as a 64-bit word goes
        w = int(ws0[i, j])
        ws[i, j] = np.uint64(M64 - (M64 - w) % q)
    ws[0, 0] = np.uint64(M64 - (M64 - int(ws0[0, 0])) % q)               # and one public word
    assert (ws % np.uint64(q) == ws0).all() and (ws[:, :N_PUBLIC] >= q).all() and int(ws.max()) > M64 - q
    prover = open_prover(m, n, mats, q)
    check_stages(prover, ws, evals, coefs, quots)
    seeds = np.array([5, 6, 7, 8], dtype=np.uint64)
    for blind in (None, blinding_words(q, batch, 11)):
        check_proofs(pkg, ctx, prover, mats, m, q, ws, rows_l, range(batch), seeds, blind)


# ---- d. directed evaluation vectors through the selector circuit ------------------------------------------------------------
def directed_vectors(m, q):
    rng = np.random.default_rng(m + q % 1013)
    vecs = [[q - 1] * m, [(q - 1) * (i & 1) for i in range(m)], [(q - 1) * (1 - (i & 1)) for i in range(m)]]
    for at in sorted({0, 15, 16, 63, 64, m - 1}):
        if at < m:
            vecs.append([(q - 1) * (i == at) for i in range(m)])
    vecs.append([int(v) % q for v in rng.integers(0, 2**64, size=m, dtype=np.uint64)])
    return vecs


@pytest.mark.gpu
@pytest.mark.parametrize("m", [64, 65, 129])
@pytest.mark.parametrize("q", [Q64, QC, Q63, 16381])
def test_directed_vectors_and_the_steered_instance(pkg, ctx, open_prover, m, q):
    n, *mats = ld.selector_circuit(m)
    prover = open_prover(m, n, mats, q)
    rows_l = lo.interpolation_rows(m, q)
    vecs = directed_vectors(m, q)
    K = len(vecs)
    want = lo.interpolate_many(vecs, q, rows_l)
    ws = np.stack([ld.selector_witness(vecs[k], vecs[(k + 1) % K], vecs[(k + 2) % K]) for k in range(K)])   # each vector as A, B and C
    got_e, got_c = prover.compute_constraint_evals(ws), prover.interpolate_batch(ws)
    for k in range(K):
        for s in range(3):
            assert ints(got_e[s][k]) == vecs[(k + s) % K], (k, s)
            assert ints(got_c[s][k]) == want[(k + s) % K], (k, s)
    a, b, c = ld.steered(m, q)
    instances = [(a, b, c)]
    if q == Q64 and m < 129:
        instances.append(ld.carry_instance(m, q)[0])
    for evals in instances:
        w = ld.selector_witness(*evals)[None, :]
        coefs = lo.interpolate_many(evals, q, rows_l)
        if evals[0] is a:
            assert coefs[0] == coefs[1] == [q - 1] * m
        qq = lo.quotient(evals, q, rows_l)
        check_stages(prover, w, [list(evals)], [coefs], [qq])
        for blind in (None, np.array([M64], dtype=np.uint64)):
            check_proofs(pkg, ctx, prover, mats, m, q, w, rows_l, [0], np.array([77], dtype=np.uint64), blind)


# ---- e. the largest sums at m = 8192 ----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("q", [Q64, Q63])
def test_m8192_steered_and_random_by_polynomial_identity(pkg, ctx, open_prover, q):
    import torch
    m, batch = 8192, 2
    n, *mats = ld.selector_circuit(m)
    rng = np.random.default_rng(q % 1019)
    ra, rb = ([int(v) % q for v in rng.integers(0, 2**64, size=m, dtype=np.uint64)] for _ in range(2))
    evals = [ld.steered(m, q), (ra, rb, [x * y % q for x, y in zip(ra, rb)])]
    ws = np.stack([ld.selector_witness(*e) for e in evals])
    prover = open_prover(m, n, mats, q)
    coefs = prover.interpolate_batch(ws)
    quot, lens = prover.quotient_batch(ws)
    assert (lens >= 1).all()
    for k in range(2):
        assert (coefs[k][0] == np.uint64(q - 1)).all()                   # the steered A and B, word for word
    for i in range(batch):
        for x in (int(v) % q for v in rng.integers(0, 2**64, size=2, dtype=np.uint64)):
            at = [lo.eval_poly(coefs[k][i], x, q) for k in range(3)]
            assert at == [ld.interpolant_at(evals[i][k], x, q) for k in range(3)], (i, x)
            assert (at[0] * at[1] - at[2]) % q == lo.eval_poly(quot[i, :lens[i]], x, q) * lo.eval_vanishing(m, x, q) % q, (i, x)
    rows, proofs, _, status = prover.prove_batch(ctx, ws, np.array([1, 2], dtype=np.uint64), N_PUBLIC, ctx.modulus())
    assert np.array_equal(status, lens)
    assert list(pkg.verify_r1cs_batch(m, ws[:, :N_PUBLIC], rows, proofs, modulus=q)) == [1, 1]
    dres = torch.zeros(batch, dtype=torch.int32, device="cuda")
    dp, dr, dpr = to_dev(torch, ws[:, :N_PUBLIC]), to_dev(torch, rows), to_dev(torch, proofs)
    pkg.verify_r1cs_batch_device(m, dp.data_ptr(), N_PUBLIC, dr.data_ptr(), rows.shape[1], dpr.data_ptr(), batch, dres.data_ptr(), modulus=q,
                                 stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert list(dres.cpu().numpy()) == [1, 1]


# ---- f. the device and host verifiers against the Python verifier ------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("zk", [False, True])
@pytest.mark.parametrize("q", [Q64, QC])
def test_verifiers_equal_the_python_verifier_on_the_tamper_matrix(pkg, ctx, open_prover, q, zk):
    import torch
    m, batch = 17, 6
    n, mats, ws, *_ = random_case(m, q, batch)
    prover = open_prover(m, n, mats, q)
    blind = np.random.default_rng(17).integers(0, 2**64, size=batch, dtype=np.uint64) if zk else None
    rows, proofs, _, status = prover.prove_batch(ctx, ws, np.arange(1, batch + 1, dtype=np.uint64), N_PUBLIC, ctx.modulus(), blinding=blind)
    assert (status >= 1).all()
    pub = np.ascontiguousarray(ws[:, :N_PUBLIC])
    cases = [(rows, proofs)]
    for w in range(13):
        for val in (None, q, M64):
            p = proofs.copy()
            p[w % batch, w] = np.uint64(val) if val is not None else p[w % batch, w] ^ np.uint64(2)
            cases.append((rows, p))
    r2 = rows.copy(); r2[1, 7] ^= np.uint64(1); cases.append((r2, proofs))
    dpub = to_dev(torch, pub)
    accepted = 0
    for rr, pp in cases:
        want = [lo.verify(ints(pp[i]), ints(pub[i]), rr[i], m, q, zk) for i in range(batch)]
        assert list(pkg.verify_r1cs_batch(m, pub, rr, pp, zk=zk, modulus=q)) == want
        dres = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
        drows, dpr = to_dev(torch, rr), to_dev(torch, pp)
        pkg.verify_r1cs_batch_device(m, dpub.data_ptr(), N_PUBLIC, drows.data_ptr(), rr.shape[1], dpr.data_ptr(), batch, dres.data_ptr(), zk=zk,
                                     stream=torch.cuda.current_stream().cuda_stream, modulus=q)
        torch.cuda.synchronize()
        assert list(dres.cpu().numpy()) == want
        accepted += sum(want)
    assert accepted >= batch and accepted < batch * len(cases)            # the untouched batch passes, tampering is noticed
