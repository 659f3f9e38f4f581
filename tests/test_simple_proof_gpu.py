"""GPU suite: lsr_simple_prove_batch[_device] and lsr_simple_verify_batch[_device] against the one-by-one sequence of
the reference — random_blinding, Commitment::new, Challenge::derive, generate_opening, verify_simple — restated by
tests/simple_oracle.py, with the commitments made by pkg.Commitment."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simple_oracle as so  # noqa: E402

CQ = 17592186044417                     # Params.q: Rust's LweContext::modulus(), the commit_modulus
P44 = (1 << 44) + 1                     # the field modulus of the reference's prover tests
GOLD = 18446744069414584321
LENGTHS = [1, 4, 63, 64, 65, 4096, 5000]   # both sides of the lane / wavefront threshold (64) and of the ring degree (4096)
MODES = ["plain", "zk", "simulate"]


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.LweContext(pkg.Params(q=CQ, n=4096, k=2, sigma=3.19), key_seed=0x51AB)
    yield c
    c.close()


@pytest.fixture(scope="module")
def prover(pkg):
    p = pkg.SimpleProver(P44)
    yield p
    p.close()


def commit_fn(pkg, ctx):
    def commit(msg, seed):
        com = pkg.Commitment(ctx, np.array([int(v) % ctx.modulus() for v in msg], dtype=np.uint64), int(seed))
        words = com.as_words().copy()
        com.free()
        return words
    return commit


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def from_dev(t):
    return t.cpu().numpy().view(np.uint64)


def make_inputs(mode, length, n_public, batch, q, seed=0):
    rng = np.random.default_rng(seed + length * 3 + n_public + len(mode))
    w = None if mode == "simulate" else rng.integers(0, 2**64, size=(batch, length), dtype=np.uint64)
    pub = rng.integers(0, 2**64, size=(batch, n_public), dtype=np.uint64)
    seeds = rng.integers(1, 2**64, size=batch, dtype=np.uint64)
    bseeds = [0, 2**64 - 1, 42, 7][:batch]
    return w, pub, seeds, bseeds


def run_device(pkg, torch, ctx, prover, mode, w, pub, seeds, keys, length):
    batch = seeds.size
    W = ctx.commitment_words
    dw = None if w is None else to_dev(torch, w)
    dpub = to_dev(torch, pub) if pub.size else None
    dk = None if keys is None else to_dev(torch, keys)
    drows = torch.zeros((batch, W), dtype=torch.int64, device="cuda")
    dco = torch.zeros((batch, length), dtype=torch.int64, device="cuda")
    dpr = torch.zeros((batch, 3), dtype=torch.int64, device="cuda")
    dh = torch.zeros((batch, 32), dtype=torch.uint8, device="cuda")
    prover.prove_batch_device(ctx, None if dw is None else dw.data_ptr(), length, batch, None if dpub is None else dpub.data_ptr(), pub.shape[1], seeds,
                              ctx.modulus(), drows.data_ptr(), dco.data_ptr(), dpr.data_ptr(), dh.data_ptr(), mode=mode,
                              d_blinding_keys=None if dk is None else dk.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return from_dev(drows), from_dev(dco), from_dev(dpr), dh.cpu().numpy()


@pytest.mark.parametrize("n_public", [0, 2])
@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("mode", MODES)
def test_prove_host_and_device_match_the_oracle(pkg, ctx, prover, mode, length, n_public):
    import torch
    batch = 2
    w, pub, seeds, bseeds = make_inputs(mode, length, n_public, batch, P44)
    keys = None if mode == "plain" else pkg.chacha20rng_keys(bseeds)
    rows, coeffs, proofs, hashes = prover.prove_batch(ctx, w, pub, seeds, ctx.modulus(), mode=mode, blinding_keys=keys, length=length)
    commit = commit_fn(pkg, ctx)
    for i in range(batch):
        row, f, proof, h = so.prove_one(mode, P44, commit, [int(v) for v in pub[i]], seeds[i], length, None if w is None else w[i], bseeds[i])
        assert np.array_equal(rows[i], row), i
        assert [int(v) for v in coeffs[i]] == f, i
        assert [int(v) for v in proofs[i]] == proof, i
        assert bytes(hashes[i]) == h
    assert list(pkg.verify_simple_batch(P44, pub, rows, proofs, coeffs)) == [1] * batch
    d = run_device(pkg, torch, ctx, prover, mode, w, pub, seeds, keys, length)
    for got, want in zip(d, (rows, coeffs, proofs, hashes)):
        assert np.array_equal(got, want)


@pytest.mark.parametrize("q", [17592169062401, 97, 3, GOLD, (1 << 64) - 59])
@pytest.mark.parametrize("length", [5, 100])
def test_other_moduli(pkg, ctx, q, length):
    p = pkg.SimpleProver(q)
    assert p.modulus == q
    w, pub, seeds, bseeds = make_inputs("zk", length, 1, 3, q)
    keys = pkg.chacha20rng_keys(bseeds)
    rows, coeffs, proofs, hashes = p.prove_batch(ctx, w, pub, seeds, ctx.modulus(), mode="zk", blinding_keys=keys)
    commit = commit_fn(pkg, ctx)
    for i in range(3):
        row, f, proof, h = so.prove_one("zk", q, commit, [int(pub[i, 0])], seeds[i], length, w[i], bseeds[i])
        assert np.array_equal(rows[i], row) and [int(v) for v in coeffs[i]] == f and [int(v) for v in proofs[i]] == proof and bytes(hashes[i]) == h
    assert list(pkg.verify_simple_batch(q, pub, rows, proofs, coeffs)) == [1, 1, 1]
    p.close()


def test_seed_zero_fresh_entropy_and_refusals(pkg, ctx, prover):
    import torch
    length, batch = 70, 3
    w, pub, seeds, bseeds = make_inputs("zk", length, 2, batch, P44)
    keys = pkg.chacha20rng_keys(bseeds)
    zs = seeds.copy(); zs[1] = 0
    rows, coeffs, proofs, _ = prover.prove_batch(ctx, w, pub, zs, ctx.modulus(), mode="zk", blinding_keys=keys)
    ref = prover.prove_batch(ctx, w, pub, seeds, ctx.modulus(), mode="zk", blinding_keys=keys)
    assert list(pkg.verify_simple_batch(P44, pub, rows, proofs, coeffs)) == [1] * batch
    assert int(proofs[1, 2]) == 0 and np.array_equal(coeffs, ref[1])
    assert np.array_equal(np.delete(rows, 1, 0), np.delete(ref[0], 1, 0))
    fresh = prover.prove_batch(ctx, w, pub, seeds, ctx.modulus(), mode="zk")               # blinding keys from OS entropy
    assert list(pkg.verify_simple_batch(P44, pub, fresh[0], fresh[2], fresh[1])) == [1] * batch
    assert not np.array_equal(fresh[1], ref[1])
    with pytest.raises(pkg.CoreError, match="seed 0"):
        run_device(pkg, torch, ctx, prover, "zk", w, pub, zs, keys, length)
    with pytest.raises(pkg.CoreError, match="blinding keys"):
        run_device(pkg, torch, ctx, prover, "zk", w, pub, seeds, None, length)
    with pytest.raises(pkg.CoreError, match="odd"):
        pkg.SimpleProver(1 << 44)


def test_random_blinding_device_equals_host(pkg):
    import torch
    batch, length = 4096, 4096
    keys = pkg.chacha20rng_keys(np.arange(batch, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
    host = pkg.random_blinding(keys, length, P44)
    dk = to_dev(torch, keys)
    out = torch.zeros((batch, length), dtype=torch.int64, device="cuda")
    pkg.random_blinding_device(dk.data_ptr(), batch, length, P44, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(from_dev(out), host)
    small = torch.zeros((3, 9), dtype=torch.int64, device="cuda")
    pkg.random_blinding_device(dk.data_ptr(), 3, 9, 97, small.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(from_dev(small), pkg.random_blinding(keys[:3], 9, 97))


def tamper_cases(rows, coeffs, proofs, pub, q):
    cases = [(rows, coeffs, proofs, pub)]
    p = proofs.copy(); p[0, 0] ^= np.uint64(1); cases.append((rows, coeffs, p, pub))
    p = proofs.copy(); p[1, 1] = np.uint64(q); cases.append((rows, coeffs, p, pub))
    p = proofs.copy(); p[2, 1] = np.uint64((int(p[2, 1]) + 1) % q); cases.append((rows, coeffs, p, pub))
    c = coeffs.copy(); c[3, -1] ^= np.uint64(8); cases.append((rows, c, proofs, pub))
    c = coeffs.copy(); c[0, 0] = np.uint64(int(c[0, 0]) + q); cases.append((rows, c, proofs, pub))     # congruent: still valid
    r = rows.copy(); r[1, 9] ^= np.uint64(1); cases.append((r, coeffs, proofs, pub))
    u = pub.copy(); u[2, 0] ^= np.uint64(1); cases.append((rows, coeffs, proofs, u))
    return cases


@pytest.mark.parametrize("length", [4, 64, 65, 1000])
def test_device_verify_equals_host_verify(pkg, ctx, prover, length):
    import torch
    batch = 5
    w, pub, seeds, _ = make_inputs("plain", length, 1, batch, P44)
    rows, coeffs, proofs, _ = prover.prove_batch(ctx, w, pub, seeds, ctx.modulus())
    for rr, cc, pp, uu in tamper_cases(rows, coeffs, proofs, pub, P44):
        host = pkg.verify_simple_batch(P44, uu, rr, pp, cc)
        want = [so.verify_one(P44, [int(uu[i, 0])], rr[i], pp[i], [int(v) for v in cc[i]]) for i in range(batch)]
        assert list(host) == want
        dres = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
        du, dr, dc, dp = to_dev(torch, uu), to_dev(torch, rr), to_dev(torch, cc), to_dev(torch, pp)
        pkg.verify_simple_batch_device(P44, du.data_ptr(), 1, dr.data_ptr(), rr.shape[1], dp.data_ptr(), dc.data_ptr(), length, batch, dres.data_ptr(),
                                       stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert list(dres.cpu().numpy()) == want


@pytest.mark.parametrize("length", [4, 100, 4096, 5000])
def test_verify_with_context_equals_verify_opening_with_context(pkg, ctx, prover, length):
    import torch
    batch = 4
    rng = np.random.default_rng(length)
    t = ctx.plain_modulus
    w = rng.integers(0, t, size=(batch, length), dtype=np.uint64)              # below t: these open
    w[1] = rng.integers(t, 2**64, size=length, dtype=np.uint64)                # field-sized words never open as given
    w[2, length // 2] = np.uint64(t + 5)
    pub = rng.integers(0, 2**64, size=(batch, 2), dtype=np.uint64)
    seeds = np.arange(11, 11 + batch, dtype=np.uint64)
    rows, coeffs, proofs, _ = prover.prove_batch(ctx, w, pub, seeds, ctx.modulus())
    commit = commit_fn(pkg, ctx)
    for rr, cc, pp, uu in tamper_cases(rows, coeffs, proofs, pub, P44)[:5]:
        want = []
        for i in range(batch):
            ok = so.verify_one(P44, [int(v) for v in uu[i]], rr[i], pp[i], [int(v) for v in cc[i]])
            com = pkg.Commitment(ctx, [int(v) % P44 for v in coeffs[i]], int(seeds[i]))   # the honest commitment: rows[i]
            assert np.array_equal(com.as_words(), rows[i])
            if ok and not np.array_equal(rr[i], rows[i]):
                ok = 0
            want.append(int(ok and pkg.verify_opening_with_context(ctx, com, [int(v) % P44 for v in cc[i]], [int(pp[i, 2])])))
            com.free()
        host = pkg.verify_simple_batch(P44, uu, rr, pp, cc, ctx=ctx)
        assert list(host) == want
        dres = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
        du, dr, dc, dp = to_dev(torch, uu), to_dev(torch, rr), to_dev(torch, cc), to_dev(torch, pp)
        pkg.verify_simple_batch_device(P44, du.data_ptr(), 2, dr.data_ptr(), rr.shape[1], dp.data_ptr(), dc.data_ptr(), length, batch, dres.data_ptr(),
                                       ctx=ctx, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert list(dres.cpu().numpy()) == want
    honest = pkg.verify_simple_batch(P44, pub, rows, proofs, coeffs, ctx=ctx)
    assert list(honest) == ([1, 0, 0, 1] if length <= 4096 else [0, 0, 0, 0])


def test_stream_capture_is_refused(pkg, ctx, prover):
    import torch
    length, batch = 16, 2
    w, pub, seeds, _ = make_inputs("plain", length, 1, batch, P44)
    rows, coeffs, proofs, _ = prover.prove_batch(ctx, w, pub, seeds, ctx.modulus())
    dw, dpub = to_dev(torch, w), to_dev(torch, pub)
    drows = torch.zeros((batch, ctx.commitment_words), dtype=torch.int64, device="cuda")
    dco = torch.zeros((batch, length), dtype=torch.int64, device="cuda")
    dpr = torch.zeros((batch, 3), dtype=torch.int64, device="cuda")
    dres = torch.zeros(batch, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g, cs = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(cs):
        with torch.cuda.graph(g, stream=cs):
            with pytest.raises(pkg.CoreError, match="capturable"):
                prover.prove_batch_device(ctx, dw.data_ptr(), length, batch, dpub.data_ptr(), 1, seeds, ctx.modulus(), drows.data_ptr(), dco.data_ptr(),
                                          dpr.data_ptr(), stream=cs.cuda_stream)
            with pytest.raises(pkg.CoreError, match="capturable"):
                pkg.verify_simple_batch_device(P44, dpub.data_ptr(), 1, drows.data_ptr(), ctx.commitment_words, dpr.data_ptr(), dco.data_ptr(), length, batch,
                                               dres.data_ptr(), stream=cs.cuda_stream)
    torch.cuda.synchronize()
    assert list(pkg.verify_simple_batch(P44, pub, rows, proofs, coeffs)) == [1, 1]
