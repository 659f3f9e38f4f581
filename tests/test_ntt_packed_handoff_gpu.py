"""The two-pass transform of the f64 flavour (n = 2^13 ... 2^17) may hand its private intermediate from one pass to the other in
6 bytes per residue instead of 8 (DESIGN.md §3, §4 "6-byte hand-off"): admissible when (8 + 7 r_top) q < 2^50, r_top = 4 stages in
the strided round for n <= 2^16 and 5 for n = 2^17, and not switched off with LAMBDA_SNARK_NTT_HANDOFF=8 when the context is made.
Only the representation of the intermediate changes, so every word of the results is compared: with the CPU oracle, and with a
context on the 8-byte path.  Each case asserts lsr_ntt_handoff_bytes, so it cannot pass on the wrong path.

`pre` (the fused diagonal multiply) exists for NTT_MODULUS contexts only and never meets the packed path."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N16 = 65536
Q16 = 17592182243329          # the benchmark's modulus (bench.py): 44 bits, q = 1 mod 2^17
Q44 = 17592180539393          # the largest prime below 2^44 with q = 1 mod 2^18 (n = 2^13 and n = 2^17 alike)
BOUND4 = (2**50 - 1) // 36    # largest q with (8 + 7 * 4) q < 2^50: the four-stage hand-off fits 48 bits


def is_prime(m):
    """Miller-Rabin, deterministic below 3.3 * 10^24 with these bases."""
    if m < 2:
        return False
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41):
        if m % p == 0:
            return m == p
    d, s = m - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41):
        x = pow(a, d, m)
        if x in (1, m - 1):
            continue
        for _ in range(s - 1):
            x = x * x % m
            if x == m - 1:
                break
        else:
            return False
    return True


def ntt_prime(start, step_sign, n):
    """the NTT-friendly prime (q = 1 mod 2n) nearest to `start` on its lower (step_sign = -1, start included) or upper (+1, start
    excluded) side"""
    m = 2 * n
    q = start - (start - 1) % m if step_sign < 0 else start + m - (start - 1) % m
    while not is_prime(q):
        q += step_sign * m
    return q


Q_BELOW = ntt_prime(BOUND4, -1, N16)      # the largest admissible modulus at n = 2^16
Q_ABOVE = ntt_prime(BOUND4, +1, N16)      # the smallest inadmissible one


def test_bound_primes():
    assert 36 * Q_BELOW < 2**50 <= 36 * Q_ABOVE and Q_ABOVE < 2**45
    assert 36 * Q16 < 2**50 and (8 + 7 * 5) * Q44 < 2**50
    for q in (Q_BELOW, Q_ABOVE):
        assert is_prime(q) and (q - 1) % (2 * N16) == 0


def pattern_rows(oracle, q, n, batch):
    """name -> [batch, n] inputs: splitmix as in bench.py (polynomial i from seed 0xDEADBEEF + i), all zero, all q - 1, q - 1 on
    even and 0 on odd indices, a single q - 1 at index 0 and at index n - 1.  The constant and alternating rows drive the hand-off
    words towards their largest magnitudes, and between them the rows exercise both signs of the halfword."""
    top = np.uint64(q - 1)
    one = {
        "zero": np.zeros(n, np.uint64),
        "top": np.full(n, top, np.uint64),
        "even_top": np.where(np.arange(n) % 2 == 0, top, np.uint64(0)).astype(np.uint64),
        "spike_first": np.zeros(n, np.uint64),
        "spike_last": np.zeros(n, np.uint64),
    }
    one["spike_first"][0] = top
    one["spike_last"][n - 1] = top
    rows = {name: np.ascontiguousarray(np.broadcast_to(row, (batch, n))) for name, row in one.items()}
    rows["splitmix"] = np.stack([oracle.splitmix(0xDEADBEEF + i, q, n) for i in range(batch)])
    return rows


def check_against_oracle(ctx, oracle, q, n, rows):
    for name, a in rows.items():
        f = ctx.forward_batch(a)
        assert np.array_equal(f, oracle.ntt_forward(q, n, a)), (q, n, name, "forward")
        assert np.array_equal(ctx.inverse_batch(f), a), (q, n, name, "round trip")


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("q", [Q16, Q_BELOW], ids=["bench_modulus", "largest_admissible"])
def test_packed_matches_oracle(pkg, oracle, q, batch):
    ctx = pkg.NttContext(q, N16)
    assert ctx.uses_f64 and ctx.handoff_bytes == 6
    check_against_oracle(ctx, oracle, q, N16, pattern_rows(oracle, q, N16, batch))
    ctx.close()


@pytest.mark.parametrize("batch", [1, 3])
def test_modulus_above_the_bound_keeps_eight_bytes(pkg, oracle, batch):
    ctx = pkg.NttContext(Q_ABOVE, N16)
    assert ctx.uses_f64 and ctx.handoff_bytes == 8
    check_against_oracle(ctx, oracle, Q_ABOVE, N16, pattern_rows(oracle, Q_ABOVE, N16, batch))
    ctx.close()


def test_no_handoff_at_single_pass_sizes(pkg):
    ctx = pkg.NttContext(Q16, 4096)
    assert ctx.handoff_bytes == 8
    ctx.close()


@pytest.fixture()
def context_pair(pkg, monkeypatch):
    """contexts on one modulus, the second created under LAMBDA_SNARK_NTT_HANDOFF=8 (read at creation: one process holds both)"""
    made = []

    def make(q, n):
        packed = pkg.NttContext(q, n)
        monkeypatch.setenv("LAMBDA_SNARK_NTT_HANDOFF", "8")
        plain = pkg.NttContext(q, n)
        monkeypatch.delenv("LAMBDA_SNARK_NTT_HANDOFF")
        assert packed.handoff_bytes == 6 and plain.handoff_bytes == 8
        made.extend([packed, plain])
        return packed, plain

    yield make
    for ctx in made:
        ctx.close()


def test_two_contexts_agree_word_for_word(oracle, context_pair):
    packed, plain = context_pair(Q16, N16)
    a = np.stack([oracle.splitmix(0xDEADBEEF + i, Q16, N16) for i in range(3)])
    f6, f8 = packed.forward_batch(a), plain.forward_batch(a)
    assert np.array_equal(f6, f8)
    # inverse of operands that are not a transform of this library's own making as well
    assert np.array_equal(packed.inverse_batch(a), plain.inverse_batch(a))
    assert np.array_equal(packed.inverse_batch(f6), a) and np.array_equal(plain.inverse_batch(f8), a)


CHUNK_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import __graft_entry__ as entry
import oracle_binding
pkg, orc = entry.load_package(), oracle_binding.load()
q, n, batch = {q}, {n}, 5
ctx = pkg.NttContext(q, n)
assert ctx.handoff_bytes == 6, ctx.handoff_bytes
a = np.stack([orc.splitmix(0xDEADBEEF + i, q, n) for i in range(batch)])
a[3, :] = q - 1
f = ctx.forward_batch(a)
assert np.array_equal(f, orc.ntt_forward(q, n, a)), "forward"
assert np.array_equal(ctx.inverse_batch(f), a), "round trip"
ctx.close()
print("chunks ok")
"""


def test_batch_over_two_chunks_with_ragged_tail(pkg):
    """LAMBDA_SNARK_NTT_CHUNK_MIB is read once per process: a child with 1 MiB chunks (2 polynomials at n = 2^16) walks 5
    polynomials as 2 + 2 + 1"""
    env = dict(os.environ, LAMBDA_SNARK_NTT_CHUNK_MIB="1")
    env.pop("LAMBDA_SNARK_NTT_HANDOFF", None)
    code = CHUNK_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), q=Q16, n=N16)
    done = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert done.returncode == 0 and "chunks ok" in done.stdout, done.stdout[-2000:]


@pytest.mark.parametrize("n,batch", [(8192, 3), (131072, 1)], ids=["smallest_two_pass", "five_stage_round"])
def test_other_two_pass_sizes(pkg, oracle, n, batch):
    """the LT = 9 tile pass (a wavefront's row is two half cells) and the five-stage strided round of n = 2^17 come out of the same
    templates; random and all-(q - 1) inputs"""
    ctx = pkg.NttContext(Q44, n)
    assert ctx.uses_f64 and ctx.handoff_bytes == 6
    rows = {"splitmix": np.stack([oracle.splitmix(0xDEADBEEF + i, Q44, n) for i in range(batch)]),
            "top": np.full((batch, n), Q44 - 1, np.uint64)}
    check_against_oracle(ctx, oracle, Q44, n, rows)
    ctx.close()


def test_largest_admissible_modulus_of_the_five_stage_round(pkg, oracle):
    """n = 2^17 as test_packed_matches_oracle at n = 2^16: the largest prime q = 1 mod 2^18 with (8 + 7 * 5) q < 2^50 reports 6 bytes
    and matches the oracle on the same inputs"""
    n = 131072
    q = ntt_prime((2**50 - 1) // 43, -1, n)
    assert 43 * q < 2**50 and is_prime(q) and (q - 1) % (2 * n) == 0
    ctx = pkg.NttContext(q, n)
    assert ctx.uses_f64 and ctx.handoff_bytes == 6
    check_against_oracle(ctx, oracle, q, n, pattern_rows(oracle, q, n, 1))
    ctx.close()


def test_five_stage_bound(pkg):
    """n = 2^17 runs five strided stages: (8 + 7 * 5) q < 2^50.  Q_BELOW is admissible for four stages only (and is 1 mod 2^18 or
    not by chance), so the bound is checked where the library decides it, on a modulus that hosts both sizes."""
    q = ntt_prime((2**50 - 1) // 43, +1, 131072)
    assert q < BOUND4
    wide, narrow = pkg.NttContext(q, 131072), pkg.NttContext(q, N16)
    assert wide.handoff_bytes == 8 and narrow.handoff_bytes == 6
    wide.close()
    narrow.close()


def test_out_of_place_source_through_the_packed_path(oracle, context_pair):
    """a ring multiply by one shared b transforms b out of place (launch_ntt with a source array) through the context's two-pass
    path; the product must be the same words on both hand-offs"""
    packed, plain = context_pair(Q16, N16)
    a = np.stack([oracle.splitmix(0xA0 + i, Q16, N16) for i in range(2)])
    b = oracle.splitmix(0xB0, Q16, N16)
    b[::3] = Q16 - 1
    assert np.array_equal(packed.ring_mul(a, b), plain.ring_mul(a, b))


def test_added_residues_through_the_packed_path(pkg, oracle, monkeypatch):
    """u = INTT(a_hat o NTT(r)) + e1 through the unfused pipeline: its inverse is the two-pass inverse with e1 added in the strided
    round's final store.  Against the oracle, and word for word against a context on the 8-byte path."""
    import torch
    monkeypatch.setenv("LAMBDA_SNARK_COMMIT_FUSED", "0")
    q, n, batch = Q16, N16, 3
    r = np.stack([oracle.splitmix(0xC0 + i, q, n) for i in range(batch)])
    e1 = oracle.splitmix(0xE1, q, batch * n).reshape(batch, n)
    e1[0, :] = q - 1
    e1[1, ::2] = 0
    s = torch.cuda.current_stream().cuda_stream
    got = {}
    for want_bytes in (6, 8):
        if want_bytes == 8:
            monkeypatch.setenv("LAMBDA_SNARK_NTT_HANDOFF", "8")
        lctx = pkg.LweContext(pkg.Params(q=q, n=n, k=1, sigma=3.19), key_seed=0xD0)
        assert lctx._lib.lsr_ntt_handoff_bytes(lctx._lib.lsr_lwe_ntt_context(lctx.handle)) == want_bytes
        d_r = torch.from_numpy(r.view(np.int64)).cuda()
        d_e1 = torch.from_numpy(e1.view(np.int64)).cuda()
        d_u = torch.empty_like(d_r)
        assert lctx._lib.lsr_mlwe_matvec_batch_device(lctx.handle, d_r.data_ptr(), d_e1.data_ptr(), d_u.data_ptr(), batch, None, s) == 0
        torch.cuda.synchronize()
        got[want_bytes] = d_u.cpu().numpy().view(np.uint64)
        if want_bytes == 6:
            a_hat = lctx.public_matrix()
            for j in range(batch):
                assert np.array_equal(got[6][j], oracle.mlwe_matvec(q, n, 1, a_hat, r[j].reshape(1, n), e1[j].reshape(1, n))[0]), j
        lctx.close()
    assert np.array_equal(got[6], got[8])
