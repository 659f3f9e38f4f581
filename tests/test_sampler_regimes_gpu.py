"""Every CDT table regime of the in-kernel Gaussian samplers (lsr_sampler.hpp), at every site that inlines them.

The sampler turns a uniform word into a magnitude in one of three ways, chosen by the number of table entries that
gaussian_scan_entries keeps: a 5-step search over a table held in lanes 0..31 (<= 32 entries), a 6-step search with a second
register pair (33..64), and a linear scan over an LDS copy of the table (> 64).  The sampled strided rounds of the n = 2^16 / 2^17
matrix-vector product split once more at 127 entries: up to there the forward round draws half of the rows into an int8 side slot,
above everything is drawn in the inverse round.  sigma = 3.45 / 3.5 / 6.9 / 7.0 / 13.9 / 14.0 sit on the two sides of the three
limits (32 | 33, 64 | 65, 127 | 128 entries); every case derives the entry count from the oracle's table and asserts it, so a
drifted sigma fails instead of testing another regime.  All comparisons are exact.

  part 1  lsr_mlwe_matvec_batch_device with e1 sampled inside the strided rounds, against oracle.mlwe_matvec and the e1-given route
  part 2  whole commitments (lsr_lwe_commit_rows_device) on the tile, fused, fused-matvec and general pipelines, against
          oracle.lwe_commit and a same-key context on the general kernels; openings; decode with the measured noise
  part 3  two-prime RNS contexts (rns-tile / rns-general) against the oracle under each prime
"""
import functools

import numpy as np
import pytest

from test_commit_rows_gpu import _keys, _rows_device
from test_rns_commit_gpu import _check_row_against_oracle, _device_rows

pytestmark = pytest.mark.gpu

KEY = 0x1234ABCD
RNS_KEY = 77
# sigma -> scanned table entries (gaussian_cdf / gaussian_scan_entries restated in 80-bit arithmetic; asserted against the oracle's
# table in every case)
ENTRIES = {3.45: 32, 3.5: 33, 6.9: 64, 7.0: 65, 13.9: 127, 14.0: 128}
SATURATED = np.uint64(2**63 - 1)


def scanned_entries(oracle, sigma):
    """gaussian_scan_entries on the oracle's table: index of the first entry whose upper 63 bits are all ones, plus one, capped at the
    table length."""
    cdf = oracle.gaussian_cdf(sigma)
    saturated = np.flatnonzero((cdf >> np.uint64(1)) == SATURATED)
    return min(cdf.size, int(saturated[0]) + 1) if saturated.size else cdf.size


def regime(oracle, sigma):
    """the entry count of sigma, asserted to be the one the case was written for"""
    entries = scanned_entries(oracle, sigma)
    assert entries == ENTRIES[sigma], f"sigma {sigma} scans {entries} table entries, the case needs {ENTRIES[sigma]}"
    return entries


# The upper half of a 33..64-entry table answers only for samples of magnitude >= 32, and a wrong upper-half entry only shows at
# magnitude >= 33.  At sigma = 6.9 such a sample has probability 2.5e-6: a case with fewer than a million samples meets one only if its
# seed is chosen for it.  DEEP holds, per 64-entry case, a seed (found by scanning seeds 1, 2, ... on the oracle's streams) and where
# the sample sits: commitments (key seed, ring degree, rank) -> (seed, stream domain, polynomial, sample) for the message DEEP_MSG;
# the matrix-vector product (ring degree, rank) -> (seed, polynomial, sample).  Every case recomputes the sample on the oracle and
# asserts its magnitude.  At 33 entries (sigma = 3.5) the one upper-half entry needs a 9.1 sigma sample, probability 1e-19: no input
# reaches it, there the cases check that the six-step form gives the lower half's words.
DEEP_MAGNITUDE = 33
DEEP_MSG = np.arange(1, 10, dtype=np.uint64)
DEEP = {(65536, 3): (1, 2, 27694),
        (KEY, 4096, 2): (35, 5, 1, 3424), (KEY, 65536, 4): (2, 5, 1, 59425), (KEY, 131072, 2): (1, 5, 1, 88681),
        (RNS_KEY, 4096, 4): (29, 5, 1, 3883), (RNS_KEY, 1024, 3): (44, 4, 1, 569)}


def stream_word(oracle, key, domain, index, sample):
    """64-bit word `sample` of the stream (256-bit key as eight 32-bit words, domain, index): ChaCha20 block sample / 8, nonce
    {domain, index_lo, index_hi}, words 2 (sample % 8) and 2 (sample % 8) + 1 (lsr_sampler.hpp)"""
    block = oracle.chacha20_block(key, sample // 8, [domain, index & 0xFFFFFFFF, index >> 32])
    return int(block[2 * (sample % 8)]) | int(block[2 * (sample % 8) + 1]) << 32


def magnitude_of(oracle, sigma, word):
    """the sampler's definition: number of scanned 63-bit table entries below the word's upper 63 bits"""
    cdf = oracle.gaussian_cdf(sigma)[:scanned_entries(oracle, sigma)]
    return int(np.count_nonzero((cdf >> np.uint64(1)) < np.uint64(word >> 1)))


def deep_commit_seed(oracle, sigma, key_seed, n, k, t):
    """the seed of DEEP for this commitment case, after checking on the oracle that it draws a sample of the upper table half"""
    seed, domain, index, sample = DEEP[(key_seed, n, k)]
    ident = oracle.context_keys(key_seed)[2]
    key = oracle.commit_key(seed, ident, DEEP_MSG, t)
    assert magnitude_of(oracle, sigma, stream_word(oracle, key, domain, index, sample)) >= DEEP_MAGNITUDE
    return seed


def _close(*contexts):
    for ctx in contexts:
        if ctx is not None:
            ctx.close()


# ---- part 1: the matrix-vector product with e1 sampled in the strided rounds ----

@functools.lru_cache(maxsize=1)
def _witness(oracle, q, n, k, batch):
    """r[batch][k][n], uniform from splitmix64 seed 0xC0FFEE + j; shared by the consecutive cases of one shape, never written"""
    return np.stack([oracle.splitmix(0xC0FFEE + j, q, k * n).reshape(k, n) for j in range(batch)])


SMALL = [(65536, 3, 3, s) for s in (3.45, 3.5, 6.9, 7.0, 13.9, 14.0)]          # rank 3: poly / components, poly % components no shifts
SMALL += [(131072, k, 2, s) for k in (1, 2) for s in (3.5, 7.0, 14.0)]         # the five-stage (R = 5) rounds
CHUNKED = [(65536, 4, 70, s) for s in (7.0, 14.0)]                             # chunks of 32 / 32 / 6 vectors on two lanes


@pytest.mark.parametrize("n,k,batch,sigma", CHUNKED + SMALL)       # (the large witness array leaves the cache with the next shape)
def test_matvec_with_e1_sampled_in_the_rounds(pkg, oracle, n, k, batch, sigma):
    """u = INTT(A^T NTT(r)) + e1 with e1 drawn inside the strided rounds (seeds given, d_e1 NULL): the picked vectors (all of a small
    batch; first / last of every chunk of the 70-vector one) equal oracle.mlwe_matvec with the oracle's own e1; the whole output equals
    the e1-given route (stand-alone sampler, then the mixed / three-launch schedule) word for word; every word is canonical; r is only
    read."""
    import torch
    entries = regime(oracle, sigma)
    q = oracle.L.oracle_lwe_select_modulus(0, n)
    picks = range(batch) if batch <= 3 else (0, 31, 32, 63, 64, 69)
    ctx = pkg.LweContext(pkg.Params(q=q, n=n, k=k, sigma=sigma), key_seed=0xF00D + k)
    try:
        assert ctx.commit_modulus == q
        assert ctx.pipeline == ("fused" if entries <= 64 else "fused-matvec")
        a_hat = ctx.public_matrix()
        r = _witness(oracle, q, n, k, batch)
        seeds = (np.arange(batch, dtype=np.uint64) + np.uint64(7)) * np.uint64(0x9E3779B9)
        if entries == 64:                                       # vector 1 draws from the upper half of the table
            seeds[1], deep_poly, deep_sample = DEEP[(n, k)]
            deep = oracle.sample_gaussian_seeded(n, sigma, int(seeds[1]), 5, deep_poly)
            assert abs(int(deep[deep_sample])) >= DEEP_MAGNITUDE
        s = torch.cuda.current_stream().cuda_stream
        d_r = torch.from_numpy(r.view(np.int64)).cuda()
        d_u = torch.zeros_like(d_r)
        assert ctx._lib.lsr_mlwe_matvec_batch_device(ctx.handle, d_r.data_ptr(), None, d_u.data_ptr(), batch, seeds.ctypes.data, s) == 0
        torch.cuda.synchronize()
        assert np.array_equal(d_r.cpu().numpy().view(np.uint64), r), "r was written"
        assert int(d_u.min().item()) >= 0 and int(d_u.max().item()) < q
        for j in picks:
            e1 = np.stack([oracle.sample_gaussian_seeded(n, sigma, int(seeds[j]), 5, i) for i in range(k)])
            assert int(np.abs(e1).max()) < entries
            e1 = np.where(e1 < 0, e1 + q, e1).astype(np.uint64)
            want = oracle.mlwe_matvec(q, n, k, a_hat, r[j], e1)
            got = d_u[j].cpu().numpy().view(np.uint64)
            assert np.array_equal(got, want), (n, k, sigma, j, np.argwhere(got != want)[:8].tolist())
        d_e1 = torch.empty_like(d_r)
        assert ctx._lib.lsr_lwe_sample_blinding_device(ctx.handle, d_e1.data_ptr(), batch, seeds.ctypes.data, s) == 0
        d_given = torch.zeros_like(d_r)
        assert ctx._lib.lsr_mlwe_matvec_batch_device(ctx.handle, d_r.data_ptr(), d_e1.data_ptr(), d_given.data_ptr(), batch, None, s) == 0
        torch.cuda.synchronize()
        assert torch.equal(d_u, d_given), (n, k, sigma, torch.nonzero(d_u != d_given)[:8].tolist())
        assert np.array_equal(d_r.cpu().numpy().view(np.uint64), r), "r was written"
    finally:
        _close(ctx)


# ---- part 2: whole commitments on the tile and fused paths ----

COMMITS = [(3.5, 4096, 4, "tile"), (6.9, 4096, 2, "tile"), (7.0, 4096, 2, "general"), (3.5, 65536, 1, "fused"),
           (6.9, 65536, 4, "fused"),            # rank 4: the scalar component as a second pass (a_perm + b_perm)
           (6.9, 131072, 2, "fused"), (7.0, 65536, 2, "fused-matvec"), (14.0, 131072, 1, "fused-matvec")]


@pytest.mark.parametrize("sigma,n,k,want", COMMITS)
def test_whole_commitments_in_every_regime(pkg, oracle, monkeypatch, sigma, n, k, want):
    """Three commitments to nine words (row 0 with words >= t, embedded mod t): every row equals oracle.lwe_commit and the row of a
    same-key context on the general kernels (LAMBDA_SNARK_COMMIT_FUSED=0, read at creation); the rows open to the embedded words and
    not to the words >= t as given (commitment.cpp:223-226); they decode to the embedded words, zero beyond, with a noise level inside
    the capacity."""
    entries = regime(oracle, sigma)
    q = oracle.L.oracle_lwe_select_modulus(0, n)
    ctx = general = None
    try:
        ctx = pkg.LweContext(pkg.Params(q=q, n=n, k=k, sigma=sigma), key_seed=KEY)
        monkeypatch.setenv("LAMBDA_SNARK_COMMIT_FUSED", "0")
        general = pkg.LweContext(pkg.Params(q=q, n=n, k=k, sigma=sigma), key_seed=KEY)
        monkeypatch.delenv("LAMBDA_SNARK_COMMIT_FUSED")
        assert (ctx.pipeline, general.pipeline) == (want, "general")
        t = ctx.plain_modulus
        rng = np.random.default_rng(int(sigma * 100) + n + k)
        batch, msg_len = 3, 9
        msgs = rng.integers(0, t, size=(batch, msg_len), dtype=np.uint64)
        msgs[0, :3] = [2**63 + 5, t, 2**64 - 1]
        seeds = rng.integers(1, 2**63, size=batch, dtype=np.uint64)
        if entries == 64:                                       # row 1 draws from the upper half of the table
            msgs[1], seeds[1] = DEEP_MSG, deep_commit_seed(oracle, sigma, KEY, n, k, t)
        keys = _keys(ctx, msgs, seeds)
        assert np.array_equal(keys, _keys(general, msgs, seeds))
        rows = _rows_device(ctx, msgs, keys).cpu().numpy().view(np.uint64)
        for j in range(batch):
            expect = oracle.lwe_commit(q, n, k, sigma, KEY, [int(x) for x in msgs[j]], int(seeds[j]))
            assert np.array_equal(rows[j], expect), (sigma, n, k, j, np.argwhere(rows[j] != expect)[:8].tolist())
        assert np.array_equal(_rows_device(general, msgs, keys).cpu().numpy().view(np.uint64), rows)
        embedded = msgs % np.uint64(t)
        for c in (ctx, general):
            assert pkg.verify_openings_words(c, rows, embedded) == [1, 1, 1]
            assert pkg.verify_openings_words(c, rows, msgs) == [0, 1, 1]
        slots, status, noise_bits = ctx.decode_rows(rows, noise=True)
        assert status.tolist() == [1, 1, 1]
        assert np.array_equal(slots[:, :msg_len], embedded) and not slots[:, msg_len:].any()
        assert all(b <= ctx.noise_capacity_bits for b in noise_bits.tolist()), (noise_bits.tolist(), ctx.noise_capacity_bits)
    finally:
        _close(ctx, general)


# ---- part 3: RNS contexts ----

RNS = [(3.5, 4096, 1, "rns-tile"), (6.9, 4096, 4, "rns-tile"), (7.0, 4096, 2, "rns-general"), (6.9, 1024, 3, "rns-general"),
       (7.0, 65536, 2, "rns-general")]


@pytest.mark.parametrize("sigma,n,k,want", RNS)
def test_rns_rows_in_every_regime(pkg, oracle, sigma, n, k, want):
    """Three rows of a two-prime context through Commitment.batch_words: under each prime u equals the oracle's single-prime commitment
    and v the oracle's plus the model's message shift; lsr_lwe_commit_rows_device from commit_keys gives the same rows; the rows
    open to the embedded words."""
    entries = regime(oracle, sigma)
    ctx = pkg.LweContext.create_rns(pkg.Params(n=n, k=k, sigma=sigma), key_seed=RNS_KEY)
    try:
        assert ctx.pipeline == want
        t = ctx.plain_modulus
        rng = np.random.default_rng(int(sigma * 100) + n + k)
        batch, msg_len = 3, 9
        msgs = rng.integers(0, t, size=(batch, msg_len), dtype=np.uint64)
        msgs[0, :3] = [2**63 + 5, t, 2**64 - 1]
        seeds = rng.integers(1, 2**63, size=batch, dtype=np.uint64)
        if entries == 64:                                       # row 1 draws from the upper half of the table
            msgs[1], seeds[1] = DEEP_MSG, deep_commit_seed(oracle, sigma, RNS_KEY, n, k, t)
        rows = pkg.Commitment.batch_words(ctx, msgs, seeds)
        for j in range(batch):
            _check_row_against_oracle(oracle, rows[j], n, k, msgs[j], int(seeds[j]), sigma=sigma, key=RNS_KEY)
        assert np.array_equal(_device_rows(ctx, msgs, ctx.commit_keys(msgs, seeds)), rows)
        assert pkg.verify_openings_words(ctx, rows, msgs % np.uint64(t)) == [1, 1, 1]
    finally:
        _close(ctx)
