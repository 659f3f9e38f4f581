"""GPU suite: circuits of 2^18 .. 2^22 constraints on the NTT path — the three-pass cyclic transforms, the quotient pipeline, the
sliced evaluation stage and whole prove calls (include/lambda_snark/prover.h).

The yardstick is the oracle (oracle/lsr_prover_oracle.c), never the library's own smaller sizes: its cyclic transforms, eval_poly and
sparse product, and — because its quotient is schoolbook O(m^2) — the O(m log m) quotient of test_large_circuit_abi.py, which is built
from those transforms and Python integers and pinned there against the oracle's quotient.  Every comparison is bit-exact.

The oracle half runs on one CPU core; measured, 122 s in all: transforms 57 s (of which 131 vectors at 2^18 take 17 s and 11 at 2^22
33 s), the shared circuit cases 2^18 / 2^20 / 2^22 with their quotients 3 s / 11 s / 48 s, evaluations 3 s."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prover_replay  # noqa: E402
from test_large_circuit_abi import build_circuit, fast_quotient, make_witness, sparse_mul_vec  # noqa: E402

Q = 18446744069414584321
CQ = 17592186044417            # LweContext::modulus() of the profile below
FREE = 8
INSTANCES = {18: 3, 20: 2, 22: 2}


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.LweContext(pkg.Params(q=CQ, n=4096, k=2, sigma=3.19), key_seed=0x5EED)
    yield c
    c.close()


_cases = {}


def case(oracle, lg):
    """one circuit of 2^lg constraints with INSTANCES[lg] satisfying witnesses and, per witness, the oracle's constraint evaluations,
    interpolants and quotient (computed once per module)"""
    if lg not in _cases:
        m = 1 << lg
        rng = np.random.default_rng(1000 + lg)
        n, mats = build_circuit(rng, m, free_vars=FREE)
        ws = np.stack([make_witness(oracle, rng.integers(0, 2**64, size=FREE, dtype=np.uint64), m, mats) for _ in range(INSTANCES[lg])])
        per = []
        for z in ws:
            evals = tuple(sparse_mul_vec(oracle, mat, m, z) for mat in mats)
            quot, ln, polys = fast_quotient(oracle, *evals)
            assert ln >= 1
            per.append({"evals": evals, "quot": quot, "len": ln, "polys": polys})
        _cases[lg] = (m, n, mats, ws, per)
    return _cases[lg]


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


# ---- transforms: every row of the schedule table (r_top, r_inner, lt) = 18: (4,4,10) 19: (4,4,11) 20: (4,4,12) 21: (5,4,12) 22: (5,5,12) ----
# The default 256 MiB chunk holds 128 vectors at 2^18 and 8 at 2^22 (LAMBDA_SNARK_NTT_CHUNK_MIB is read once per process), so 131 and 11
# vectors end on a ragged chunk of 3.
@pytest.mark.parametrize("lg,batch", [(18, 131), (19, 3), (20, 3), (21, 3), (22, 11)])
def test_cyclic_transforms_match_the_oracle(pkg, oracle, lg, batch):
    n = 1 << lg
    omega = oracle.prover_omega(n)
    rng = np.random.default_rng(lg)
    x = rng.integers(0, Q, size=(batch, n), dtype=np.uint64)
    x[0] = np.uint64(Q - 1)
    x[1] = 0
    x[1, n - 1] = 1
    ntt = pkg.CyclicNtt(n)
    assert ntt.omega == omega
    fwd = ntt.forward(x).reshape(batch, n)
    inv = ntt.inverse(x).reshape(batch, n)
    ntt.close()
    for i in range(batch):
        assert np.array_equal(fwd[i], oracle.cyclic_forward(x[i], Q, omega)), (lg, i)
        assert np.array_equal(inv[i], oracle.cyclic_inverse(x[i], Q, omega)), (lg, i)


def test_device_transform_order_and_ring_mul_refusal(pkg, oracle):
    """the device entry points on a large context keep the documented orders (forward: natural in, bit-reversed out) and the ring
    multiply answers -1 with a message"""
    import torch
    n, batch = 1 << 18, 2
    omega = oracle.prover_omega(n)
    x = np.random.default_rng(7).integers(0, Q, size=(batch, n), dtype=np.uint64)
    ntt = pkg.CyclicNtt(n)
    lib = pkg._abi.lib()
    d, out = to_dev(torch, x), torch.zeros((batch, n), dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    assert lib.lsr_ntt_forward_batch_device(ntt.handle, d.data_ptr(), batch, s) == 0
    assert lib.lsr_bit_reverse_device(out.data_ptr(), d.data_ptr(), 18, batch, s) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint64)
    for i in range(batch):
        assert np.array_equal(got[i], oracle.cyclic_forward(x[i], Q, omega))
    assert lib.lsr_ntt_inverse_batch_device(ntt.handle, d.data_ptr(), batch, s) == 0
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().view(np.uint64), x)
    with pytest.raises(pkg.CoreError, match="not supported"):
        ntt.ring_mul(x[0], x[1])
    ntt.close()


# ---- quotient ----
@pytest.mark.parametrize("lg,chunk_log2", [(18, 19), (20, 20)])
def test_quotient_batch_matches_the_fast_quotient(pkg, oracle, lg, chunk_log2, monkeypatch):
    m, n, mats, ws, per = case(oracle, lg)
    good = len(per)
    ea, eb, ec = (np.stack([p["evals"][k] for p in per] + [per[0]["evals"][k]]) for k in range(3))
    ec[good, m - 3] = np.uint64((int(ec[good, m - 3]) + 1) % Q)               # the last instance: one broken constraint
    plan = pkg.QuotientPlan(m)
    monkeypatch.setenv("LAMBDA_SNARK_QUOTIENT_CHUNK_LOG2", str(chunk_log2))  # 2 (2^18) / 1 (2^20) instances per pass
    small = pkg.QuotientPlan(m)
    monkeypatch.delenv("LAMBDA_SNARK_QUOTIENT_CHUNK_LOG2")
    for p in (plan, small):
        quot, lens = p.quotient_batch(ea, eb, ec)
        assert [int(v) for v in lens] == [q["len"] for q in per] + [0]
        for i in range(good):
            assert np.array_equal(quot[i], per[i]["quot"]), (lg, i)
        p.close()


def test_quotient_identity_at_2_pow_22(pkg, oracle):
    """Q(x) (x^m - 1) = A(x) B(x) - C(x) at two random points: a wrong Q of degree < m passes one point with probability <= 2m / q < 2^-40"""
    m, n, mats, ws, per = case(oracle, 22)
    ea, eb, ec = (np.stack([p["evals"][k] for p in per]) for k in range(3))
    plan = pkg.QuotientPlan(m)
    quot, lens = plan.quotient_batch(ea, eb, ec)
    plan.close()
    rng = np.random.default_rng(22)
    ev = lambda p, x: int(oracle.eval_poly(p, x, Q))
    for i, p in enumerate(per):
        ln = int(lens[i])
        assert 1 <= ln <= m - 1 and not quot[i, ln:].any() and quot[i, ln - 1] != 0
        pa, pb, pc = p["polys"]
        for x in (int(v) for v in rng.integers(0, Q, size=2, dtype=np.uint64)):
            assert ev(quot[i, :ln], x) * ((pow(x, m, Q) - 1) % Q) % Q == (ev(pa, x) * ev(pb, x) - ev(pc, x)) % Q
        assert ln == p["len"] and np.array_equal(quot[i], p["quot"])          # and word for word against the fast quotient


# ---- prove ----
def expected_proof(pkg, oracle, ctx, m, w, p, seed, n_public, r=None):
    """the reference's sequence for one witness (lib.rs:747-809; r: 877-980) on the oracle's quotient and interpolants"""
    ln = p["len"]
    if r is None:
        coeffs = p["quot"][:ln]
    else:                                                                    # poly_add(Q, r Z_H), r1cs.rs:906-922
        coeffs = np.zeros(m + 1, dtype=np.uint64)
        coeffs[:m] = p["quot"]
        coeffs[0] = (int(coeffs[0]) - r) % Q
        coeffs[m] = r % Q
        coeffs = coeffs[:int(np.flatnonzero(coeffs)[-1]) + 1] if coeffs.any() else coeffs[:1]
    com = pkg.Commitment(ctx, coeffs % np.uint64(CQ), int(seed))
    row = com.as_words().copy()
    com.free()
    alpha, ha = prover_replay.challenge_derive([int(v) for v in w[:n_public]], row, Q)
    beta, hb = prover_replay.challenge_derive([alpha], row, Q)
    pa, pb, pc = p["polys"]
    ev = lambda poly, x: int(oracle.eval_poly(poly, x, Q))
    qa, qb = ev(coeffs, alpha), ev(coeffs, beta)
    return row, [alpha, beta, qa, qb, ev(pa, alpha), ev(pb, alpha), ev(pc, alpha), ev(pa, beta), ev(pb, beta), ev(pc, beta), qa, qb, r or 0], ha + hb, ln


_host_results = {}


@pytest.mark.parametrize("lg,zk", [(18, False), (18, True), (20, False), (20, True), (22, False)])
def test_prove_batch_matches_the_one_by_one_sequence(pkg, oracle, ctx, lg, zk):
    m, n, mats, ws, per = case(oracle, lg)
    batch, n_public = len(per), 3
    seeds = np.arange(1, batch + 1, dtype=np.uint64) * np.uint64(7919 + lg)
    blind = None
    if zk:
        blind = np.random.default_rng(lg).integers(0, 2**64, size=batch, dtype=np.uint64)
        blind[0] = np.uint64(Q + 5)                                          # reduced mod p
    prover = pkg.R1csProver(m, n, *mats)
    assert prover.uses_ntt
    rows, proofs, hashes, status = prover.prove_batch(ctx, ws, seeds, n_public, ctx.modulus(), blinding=blind)
    prover.close()
    _host_results[(lg, zk)] = (seeds, blind, rows, proofs, hashes, status)
    for i in range(batch):                                                   # every instance, every word
        r = None if blind is None else int(blind[i]) % Q
        row, proof, h, ln = expected_proof(pkg, oracle, ctx, m, ws[i], per[i], seeds[i], n_public, r)
        assert status[i] == ln, (lg, i)
        assert np.array_equal(rows[i], row), (lg, i)
        assert [int(v) for v in proofs[i]] == proof, (lg, i)
        assert bytes(hashes[i]) == h
    assert list(pkg.verify_r1cs_batch(m, ws[:, :n_public], rows, proofs, zk=zk)) == [1] * batch
    bad = proofs.copy()
    bad[batch - 1, 5] ^= np.uint64(1)
    assert list(pkg.verify_r1cs_batch(m, ws[:, :n_public], rows, bad, zk=zk)) == [1] * (batch - 1) + [0]


@pytest.mark.parametrize("zk", [False, True])
def test_device_variant_equals_host_variant_at_2_pow_18(pkg, oracle, ctx, zk):
    import torch
    m, n, mats, ws, per = case(oracle, 18)
    batch, n_public = len(per), 3
    prover = pkg.R1csProver(m, n, *mats)
    if (18, zk) in _host_results:
        seeds, blind, rows, proofs, hashes, status = _host_results[(18, zk)]
    else:
        seeds = np.arange(1, batch + 1, dtype=np.uint64) * np.uint64(7919 + 18)
        blind = np.random.default_rng(18).integers(0, 2**64, size=batch, dtype=np.uint64) if zk else None
        rows, proofs, hashes, status = prover.prove_batch(ctx, ws, seeds, n_public, ctx.modulus(), blinding=blind)
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
    prover.close()
    assert np.array_equal(drows.cpu().numpy().view(np.uint64), rows)
    assert np.array_equal(dproofs.cpu().numpy().view(np.uint64), proofs)
    assert np.array_equal(dhash.cpu().numpy(), hashes.reshape(batch, 64))
    assert np.array_equal(dstat.cpu().numpy().view(np.uint32), status)


def test_constraint_evals_and_quotient_of_a_large_prover(pkg, oracle):
    m, n, mats, ws, per = case(oracle, 18)
    prover = pkg.R1csProver(m, n, *mats)
    bad = ws.copy()
    bad[1, n - 2] = np.uint64((int(bad[1, n - 2]) + 1) % Q)
    evals = prover.compute_constraint_evals(ws)
    quot, lens = prover.quotient_batch(bad)
    prover.close()
    for i, p in enumerate(per):
        for k in range(3):
            assert np.array_equal(evals[k][i], p["evals"][k])
        if i != 1:
            assert lens[i] == p["len"] and np.array_equal(quot[i], p["quot"])
    assert lens[1] == 0


# ---- evaluation ----
def test_eval_batch_device_at_2_pow_20_plus_1(pkg, oracle):
    import torch
    length, batch = (1 << 20) + 1, 2
    rng = np.random.default_rng(9)
    coeffs = rng.integers(0, 2**64, size=(batch, length), dtype=np.uint64)
    coeffs[0, -1] = np.uint64(Q - 1)
    coeffs[1, 0] = np.uint64(2**64 - 1)
    pts = np.array([[0, 1, Q - 1, int(rng.integers(0, Q, dtype=np.uint64))] for _ in range(batch)], dtype=np.uint64)
    out = torch.zeros((batch, 4), dtype=torch.int64, device="cuda")
    dc, dp = to_dev(torch, coeffs), to_dev(torch, pts)
    pkg.prover_eval_batch_device(dc.data_ptr(), length, batch, dp.data_ptr(), 4, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint64)
    for i in range(batch):
        red = coeffs[i] % np.uint64(Q)
        for k in range(4):
            assert int(got[i, k]) == int(oracle.eval_poly(red, int(pts[i, k]), Q)), (i, k)
