"""The two-pass inverse transform of the f64 flavour (n = 2^13 ... 2^17) hands the un-centred outputs of the tile pass's last round
to the strided round, which re-centres them on load ("Deferred re-centring").  Every word of the result is compared
with the CPU oracle, on operands that drive the raw hand-off to its bound (the all-sum class reaches 32 q), for 44-bit primes of the
headline's kind and for the largest prime below 2^45 the flavour admits; then the round trip, and the inverse that adds blinding
residues in its final store (the unfused commitment pipeline), which runs the same strided pass."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

Q16 = 17592182243329          # the headline modulus: 44 bits, q = 1 mod 2^17 (n <= 2^16)
Q44 = 17592180539393          # the largest prime below 2^44 with q = 1 mod 2^18 (every n here)
Q45 = 35184365273089          # the largest prime below 2^45 with q = 1 mod 2^18: the f64 flavour's range to its end
SIZES = [8192, 16384, 32768, 65536, 131072]
CASES = [(q, n) for n in SIZES for q in (Q16, Q44, Q45) if (q - 1) % (2 * n) == 0]


def stress_rows(oracle, q, n):
    """all q - 1, all 0, alternating 0 / q - 1 (both phases), one q - 1 at each of a few positions, seeded random"""
    top = np.uint64(q - 1)
    rows = [np.full(n, top, np.uint64), np.zeros(n, np.uint64),
            np.where(np.arange(n) % 2, top, np.uint64(0)).astype(np.uint64), np.where(np.arange(n) % 2, np.uint64(0), top).astype(np.uint64)]
    for at in (0, 1, 255, 256, 4095, 4096, n // 16, n // 2 - 1, n // 2, n - 1):
        spike = np.zeros(n, np.uint64)
        spike[at] = top
        rows.append(spike)
    for seed in (1, 2, 3):
        rows.append(oracle.splitmix(0x5EED0000 + seed * 131 + n, q, n))
    return np.stack(rows)


def test_cases_cover_every_size():
    assert sorted({n for _, n in CASES}) == SIZES
    assert all(q < 2**45 and q.bit_length() >= 44 for q, _ in CASES)


@pytest.mark.parametrize("q,n", CASES)
def test_inverse_matches_oracle_word_for_word(pkg, oracle, q, n):
    ctx = pkg.NttContext(q, n)
    assert ctx.uses_f64
    a = stress_rows(oracle, q, n)
    assert np.array_equal(ctx.inverse_batch(a), oracle.ntt_inverse(q, n, a))
    # the transforms of the same rows: operands of the inverse that are spread over the whole range
    f = oracle.ntt_forward(q, n, a)
    assert np.array_equal(ctx.inverse_batch(f), a)
    ctx.close()


@pytest.mark.parametrize("q,n", CASES)
def test_round_trip(pkg, oracle, q, n):
    ctx = pkg.NttContext(q, n)
    a = stress_rows(oracle, q, n)
    f = ctx.forward_batch(a)
    assert np.array_equal(f, oracle.ntt_forward(q, n, a))
    assert np.array_equal(ctx.inverse_batch(f), a)
    ctx.close()


@pytest.mark.parametrize("q,n", CASES)
def test_inverse_with_added_residues(pkg, oracle, q, n, monkeypatch):
    """u = INTT(a_hat o NTT(r)) + e1 at rank 1 through the unfused pipeline: its inverse is run_ntt's two-pass inverse with the
    residues e1 added in the strided round's final store."""
    import torch
    monkeypatch.setenv("LAMBDA_SNARK_COMMIT_FUSED", "0")
    lctx = pkg.LweContext(pkg.Params(q=q, n=n, k=1, sigma=3.19), key_seed=0xD0 + n)
    a_hat = lctx.public_matrix()
    r = stress_rows(oracle, q, n)
    batch = r.shape[0]
    e1 = oracle.splitmix(0xE1 + n, q, batch * n).reshape(batch, n)
    e1[0, :] = q - 1
    e1[1, :] = 0
    e1[2, ::2] = q - 1
    s = torch.cuda.current_stream().cuda_stream
    d_r = torch.from_numpy(r.view(np.int64)).cuda()
    d_e1 = torch.from_numpy(e1.view(np.int64)).cuda()
    d_u = torch.empty_like(d_r)
    assert lctx._lib.lsr_mlwe_matvec_batch_device(lctx.handle, d_r.data_ptr(), d_e1.data_ptr(), d_u.data_ptr(), batch, None, s) == 0
    torch.cuda.synchronize()
    got = d_u.cpu().numpy().view(np.uint64)
    for j in range(batch):
        assert np.array_equal(got[j], oracle.mlwe_matvec(q, n, 1, a_hat, r[j].reshape(1, n), e1[j].reshape(1, n))[0]), (q, n, j)
    lctx.close()
