"""GPU suite: decoding commitment rows (lsr_lwe_decode_rows_device, lsr_lwe_decode_batch_flat, lsr_lwe_decode) and the measured
noise, on every pipeline, against the committed messages, the opening check and the big-integer model of tests/decode_model.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import decode_model
import rns_model

pytestmark = pytest.mark.gpu

SIGMA = 3.19
KEY = 77
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CONTEXTS = {}


def _ctx(pkg, kind, n, k):
    """one context per (kind, n, k) for the whole module: kind = "default" (44-bit prime), "wide" (60-bit prime, u64 kernels), "rns" """
    key = (kind, n, k)
    if key not in _CONTEXTS:
        if kind == "rns":
            _CONTEXTS[key] = pkg.LweContext.create_rns(pkg.Params(n=n, k=k, sigma=SIGMA), key_seed=KEY)
        elif kind == "wide":
            _CONTEXTS[key] = pkg.LweContext(pkg.Params(q=pkg.wide_modulus(n), n=n, k=k, sigma=SIGMA), key_seed=KEY)
        else:
            _CONTEXTS[key] = pkg.LweContext(pkg.Params(n=n, k=k, sigma=SIGMA), key_seed=KEY)
    return _CONTEXTS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for ctx in _CONTEXTS.values():
        ctx.close()
    _CONTEXTS.clear()


def _big_modulus(ctx):
    """the modulus the decoded coefficient lives under: q, or Q = q1 q2"""
    pair = ctx.rns_moduli()
    return pair[0] * pair[1] if pair else ctx.commit_modulus


def _commit(ctx, msgs, msg_len, seeds):
    """rows of lsr_lwe_commit_batch_flat for the first msg_len words of every row of msgs (msg_len may be 0)"""
    msgs = np.ascontiguousarray(msgs[:, :msg_len] if msg_len else msgs[:, :1], dtype=np.uint64)
    seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
    rows = np.zeros((seeds.size, ctx.commitment_words), dtype=np.uint64)
    assert ctx._lib.lsr_lwe_commit_batch_flat(ctx.handle, msgs.ctypes.data, msg_len, seeds.size, seeds.ctypes.data, rows.ctypes.data) == 0
    return rows


def _decode_device(ctx, rows, slots, noise=True, stream=None):
    import torch
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    count = rows.shape[0]
    d_rows = torch.from_numpy(rows.view(np.int64)).cuda()
    d_msgs = torch.full((count, slots), -1, dtype=torch.int64, device="cuda")
    d_status = torch.zeros(count, dtype=torch.int32, device="cuda")
    d_bits = torch.full((count,), 77, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    ctx.decode_rows_device(d_rows.data_ptr(), count, slots, d_msgs.data_ptr(), d_status.data_ptr(), d_bits.data_ptr() if noise else None, s)
    torch.cuda.synchronize()
    return d_msgs.cpu().numpy().view(np.uint64), d_status.cpu().numpy(), d_bits.cpu().numpy().view(np.uint32) if noise else None


def _decode_single(pkg, ctx, rows, slots):
    msgs = np.zeros((rows.shape[0], slots), dtype=np.uint64)
    status, bits = [], []
    for j in range(rows.shape[0]):
        row = np.ascontiguousarray(rows[j])
        view = pkg._abi.LweCommitment(row.ctypes.data_as(pkg._abi.u64p), row.size)
        b = ctypes.c_uint32(0)
        status.append(ctx._lib.lsr_lwe_decode(ctx.handle, ctypes.byref(view), msgs[j].ctypes.data, slots, ctypes.byref(b)))
        bits.append(b.value)
    return msgs, np.array(status, dtype=np.int32), np.array(bits, dtype=np.uint32)


def _decode_all(pkg, ctx, rows, slots):
    """the three entry points, asserted equal word for word (with and without the noise output) -> (messages, status, noise_bits);
    messages and noise of a row with status -1 are unspecified and not compared"""
    dev = _decode_device(ctx, rows, slots)
    good = dev[1] == 1
    flat = ctx.decode_rows(rows, slots=slots, noise=True)
    single = _decode_single(pkg, ctx, rows, slots)
    for other in (flat, single):
        assert np.array_equal(other[1], dev[1])
        assert np.array_equal(other[0][good], dev[0][good]) and np.array_equal(other[2][good], dev[2][good])
    quiet = _decode_device(ctx, rows, slots, noise=False)
    assert np.array_equal(quiet[0][good], dev[0][good]) and np.array_equal(quiet[1], dev[1])
    flat_quiet = ctx.decode_rows(rows, slots=slots)
    assert np.array_equal(flat_quiet[0][good], dev[0][good]) and np.array_equal(flat_quiet[1], dev[1])
    return dev


def test_capacity_and_argument_refusals(pkg, lib):
    import torch
    plain, rns = _ctx(pkg, "default", 4096, 2), _ctx(pkg, "rns", 4096, 2)
    assert plain.noise_capacity_bits == decode_model.capacity_bits(plain.commit_modulus) == 43
    assert rns.noise_capacity_bits == decode_model.capacity_bits(_big_modulus(rns)) == 87
    assert _ctx(pkg, "wide", 4096, 2).noise_capacity_bits == 59
    n = 4096
    d = torch.zeros(plain.commitment_words + n + 8, dtype=torch.int64, device="cuda")
    host = np.zeros(plain.commitment_words + n, dtype=np.uint64)
    st = np.zeros(1, dtype=np.int32)
    p, h, s = d.data_ptr(), plain.handle, torch.cuda.current_stream().cuda_stream
    view = pkg._abi.LweCommitment(host.ctypes.data_as(pkg._abi.u64p), plain.commitment_words)
    refused = [
        lambda: lib.lsr_lwe_decode_rows_device(h, None, 1, 1, p, p, None, s), lambda: lib.lsr_lwe_decode_rows_device(h, p, 1, 1, None, p, None, s),
        lambda: lib.lsr_lwe_decode_rows_device(h, p, 1, 1, p, None, None, s), lambda: lib.lsr_lwe_decode_rows_device(h, p, 1, 0, p, p, None, s),
        lambda: lib.lsr_lwe_decode_rows_device(h, p, 1, n + 1, p, p, None, s),
        lambda: lib.lsr_lwe_decode_batch_flat(h, None, 1, 1, host.ctypes.data, st.ctypes.data, None),
        lambda: lib.lsr_lwe_decode_batch_flat(h, host.ctypes.data, 1, 1, None, st.ctypes.data, None),
        lambda: lib.lsr_lwe_decode_batch_flat(h, host.ctypes.data, 1, 1, host.ctypes.data, None, None),
        lambda: lib.lsr_lwe_decode_batch_flat(h, host.ctypes.data, 1, 0, host.ctypes.data, st.ctypes.data, None),
        lambda: lib.lsr_lwe_decode_batch_flat(h, host.ctypes.data, 1, n + 1, host.ctypes.data, st.ctypes.data, None),
        lambda: lib.lsr_lwe_decode(h, None, host.ctypes.data, 1, None), lambda: lib.lsr_lwe_decode(h, ctypes.byref(view), None, 1, None),
        lambda: lib.lsr_lwe_decode(h, ctypes.byref(view), host.ctypes.data, 0, None), lambda: lib.lsr_lwe_decode(h, ctypes.byref(view), host.ctypes.data, n + 1, None),
    ]
    for call in refused:
        assert not lib.lsr_lwe_context_create_rns(None, 3, -1) and b"NULL params" in lib.lsr_last_error()      # another text in between
        assert call() == -1
        assert b"lsr_lwe_decode" in lib.lsr_last_error() and b"NULL params" not in lib.lsr_last_error()
    assert lib.lsr_lwe_decode_rows_device(h, p, 0, 1, p, p, None, s) == 0
    assert lib.lsr_lwe_decode_batch_flat(h, host.ctypes.data, 0, 1, host.ctypes.data, st.ctypes.data, None) == 0


SHAPES = [("default", 4096, 1, 3, "tile"), ("default", 4096, 2, 5, "tile"), ("default", 4096, 4, 3, "tile"), ("default", 65536, 2, 3, "fused"),
          ("default", 131072, 1, 2, "fused"), ("default", 1024, 3, 3, "general"), ("default", 8192, 2, 3, "general"), ("wide", 4096, 2, 3, "general"),
          ("rns", 4096, 2, 5, "rns-tile"), ("rns", 4096, 4, 3, "rns-tile"), ("rns", 1024, 3, 3, "rns-general")]


@pytest.mark.parametrize("kind,n,k,batch,pipeline", SHAPES)
def test_fresh_commitments_decode_to_their_message(pkg, kind, n, k, batch, pipeline):
    ctx = _ctx(pkg, kind, n, k)
    assert ctx.pipeline == pipeline
    t = ctx.plain_modulus
    rng = np.random.default_rng(n + 10 * k)
    rows, want = [], []
    for length in (0, 5, n, n + 3):
        msgs = rng.integers(0, t, size=(batch, max(length, 1)), dtype=np.uint64)
        if length:
            msgs[0, 0], msgs[batch - 1, length - 1] = t + 5, 2**64 - 1          # words >= t are embedded mod t
            msgs[1, min(2, length - 1)] = 3 * t + 1
        seeds = rng.integers(1, 2**63, size=batch, dtype=np.uint64)
        rows.append(_commit(ctx, msgs, length, seeds))
        copy = min(length, n)
        expect = np.zeros((batch, n), dtype=np.uint64)
        expect[:, :copy] = msgs[:, :copy] % np.uint64(t)
        want.append(expect)
    rows, want = np.concatenate(rows), np.concatenate(want)
    capacity = ctx.noise_capacity_bits
    for slots in (1, 5, n):
        got, status, bits = _decode_all(pkg, ctx, rows, slots)
        assert np.array_equal(got, want[:, :slots]), slots
        assert status.tolist() == [1] * rows.shape[0]
        assert all(0 < b < capacity for b in bits.tolist())              # a fresh row has noise, and headroom
        if slots == 1:
            first = bits
        assert np.array_equal(bits, first)                               # the noise covers all n coefficients whatever `slots` is


def _random_canonical_rows(ctx, header_row, count, rng):
    """valid header of this context, bodies of uniformly random canonical words"""
    n, k = ctx.ring_degree, ctx.module_rank
    pair = ctx.rns_moduli()
    head = 6 if pair else 5
    rows = np.repeat(header_row[None, :], count, axis=0).copy()
    block = (k + 1) * n
    for i, q in enumerate(pair or (ctx.commit_modulus,)):
        rows[:, head + i * block:head + (i + 1) * block] = rng.integers(0, q, size=(count, block), dtype=np.uint64)
    return rows


def _verify_device(ctx, rows, claimed):
    import torch
    d_rows = torch.from_numpy(np.ascontiguousarray(rows).view(np.int64)).cuda()
    d_msgs = torch.from_numpy(np.ascontiguousarray(claimed).view(np.int64)).cuda()
    d_res = torch.zeros(rows.shape[0], dtype=torch.int32, device="cuda")
    ctx.verify_rows_device(d_rows.data_ptr(), d_msgs.data_ptr(), claimed.shape[1], rows.shape[0], d_res.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_res.cpu().tolist()


@pytest.mark.parametrize("kind,n,k", [("default", 4096, 2), ("default", 1024, 3), ("rns", 4096, 2)])
def test_decode_is_total_and_consistent_with_verify(pkg, kind, n, k):
    ctx = _ctx(pkg, kind, n, k)
    t = ctx.plain_modulus
    rng = np.random.default_rng(3 * n + k)
    header_row = _commit(ctx, np.zeros((1, 1), dtype=np.uint64), 1, [5])[0]
    rows = _random_canonical_rows(ctx, header_row, 4, rng)
    got, status, bits = _decode_all(pkg, ctx, rows, n)
    assert status.tolist() == [1] * 4 and int(got.max()) < t
    assert all(0 < b <= ctx.noise_capacity_bits for b in bits.tolist())
    for length in (1, 7, n):
        claimed = np.ascontiguousarray(got[:, :length])
        assert _verify_device(ctx, rows, claimed) == [1] * 4, length
        for j in range(4):
            flipped = claimed.copy()
            flipped[j, length - 1] = (int(flipped[j, length - 1]) + 1) % t
            assert _verify_device(ctx, rows, flipped) == [1 if i != j else 0 for i in range(4)], (length, j)


@pytest.mark.parametrize("kind,n,k", [("default", 4096, 2), ("default", 1024, 3), ("default", 65536, 2), ("wide", 4096, 2), ("rns", 4096, 2), ("rns", 1024, 3)])
def test_secret_independent_exact_model(pkg, kind, n, k):
    """u = 0 makes x = v whatever the secret is: every slot and noise_bits against the big-integer evaluation of the definitions"""
    ctx = _ctx(pkg, kind, n, k)
    t = ctx.plain_modulus
    big = _big_modulus(ctx)
    half = big // 2
    rng = np.random.default_rng(n + k)
    lattice = [rns_model.round_div(big * m, t) for m in (0, 1, 2, t // 2, t - 2, t - 1, int(rng.integers(0, t)))]
    edge = [0, 1, big - 1, big - 2, half, half - 1, half + 1]
    step = big // t
    for point in lattice:
        edge += [(point + e) % big for e in (0, 1, -1, 5, -5, 1000, -1000, step // 2, step // 2 + 1, -(step // 2), -(step // 2) - 1, step // 2 - 1)]
    xs = np.zeros((4, n), dtype=object)
    xs[0, :] = [a * b % big for a, b in zip(rng.integers(0, 2**62, size=n).tolist(), rng.integers(0, 2**62, size=n).tolist())]
    xs[0, :len(edge)] = edge
    xs[0, n - len(edge):] = edge                                     # the same values at the far end of the row
    # row 1: all zero (noise_bits 0); row 2: lattice points with small noise (few noise bits); row 3: one large rho in the last coefficient only
    xs[2, :] = [(lattice[i % len(lattice)] + (i % 7) - 3) % big for i in range(n)]
    xs[3, n - 1] = lattice[1] + step // 2 - 3
    header_row = _commit(ctx, np.zeros((1, 1), dtype=np.uint64), 1, [5])[0]
    rows = np.repeat(header_row[None, :], 4, axis=0).copy()
    pair = ctx.rns_moduli()
    head, block = (6 if pair else 5), (k + 1) * n
    rows[:, head:] = 0
    for i, q in enumerate(pair or (big,)):
        rows[:, head + i * block + k * n:head + (i + 1) * block] = (xs % q).astype(np.uint64)
    model = [[decode_model.slot_and_rho(int(x), t, big) for x in xs[j]] for j in range(4)]
    want_slots = np.array([[s for s, _ in row] for row in model], dtype=np.uint64)
    want_bits = [max(r for _, r in row).bit_length() for row in model]
    assert want_bits[1] == 0 and want_bits[2] < want_bits[3] <= ctx.noise_capacity_bits
    for slots in (7, n):
        got, status, bits = _decode_all(pkg, ctx, rows, slots)
        assert status.tolist() == [1] * 4
        assert np.array_equal(got, want_slots[:, :slots])
        assert bits.tolist() == want_bits


def _accepts(pkg, ctx, com, coeff):
    try:
        return pkg.Commitment.linear_combine(ctx, [com], [coeff])
    except pkg.CoreError:
        return None


@pytest.mark.parametrize("kind", ["default", "rns"])
def test_noise_scales_exactly(pkg, kind):
    """The all-zero message has rho_i = t |eps_i|, so a combination with the single coefficient 2^e adds exactly e noise bits.  The
    library centres coefficients mod t, so 2^e is the multiplier only while 2^e <= t/2: e runs over the exponents below that which the
    context's budget check accepts, the largest found by asking lwe_linear_combine."""
    n, k = 4096, 2
    ctx = _ctx(pkg, kind, n, k)
    t = ctx.plain_modulus
    com = pkg.Commitment(ctx, [0] * n, seed=41)
    zeros, base = com.decode(ctx, noise=True)
    assert not zeros.any() and 0 < base < ctx.noise_capacity_bits
    accepted = []
    for e in range(64):
        if 2 ** (e + 1) > t:                # beyond t/2 the centred representative of 2^e is 2^e - t: no longer a doubling
            break
        scaled = _accepts(pkg, ctx, com, 2**e)
        if scaled is None:
            break
        accepted.append(e)
        message, bits = scaled.decode(ctx, noise=True)
        assert bits == base + e, e
        if _accepts(pkg, ctx, com, 2 ** (e + 1)) is None or 2 ** (e + 2) > t:       # the largest accepted exponent
            assert base + e <= ctx.noise_capacity_bits
            assert not message.any()
        rows = scaled.as_words()[None, :]
        assert ctx.decode_rows(rows, slots=3, noise=True)[2].tolist() == [base + e]
        scaled.free()
    assert accepted and accepted == list(range(len(accepted)))
    if kind == "default":                   # the worst-case budget of a 44-bit context ends long before t/2
        assert 2 ** (accepted[-1] + 2) < t and "noise budget" in pkg._abi.last_error()
    else:
        assert 2 ** (accepted[-1] + 2) > t
    com.free()


def test_combinations_decode(pkg):
    rng = np.random.default_rng(60)
    # three terms, small coefficients (one negative), default context
    ctx = _ctx(pkg, "default", 4096, 2)
    t = ctx.plain_modulus
    msgs = [[int(x) for x in rng.integers(0, t, 6)] for _ in range(3)]
    cs = [3, t - 2, 5]
    coms = [pkg.Commitment(ctx, m, seed=100 + i) for i, m in enumerate(msgs)]
    comb = pkg.Commitment.linear_combine(ctx, coms, cs)
    expect = [sum(decode_model.centred(c, t) * m[i] for c, m in zip(cs, msgs)) % t for i in range(6)]
    got, bits = comb.decode(ctx, slots=8, noise=True)
    assert got.tolist() == expect + [0, 0] and bits < ctx.noise_capacity_bits
    assert pkg.verify_opening_with_context(ctx, comb, expect)
    # sixteen full-range coefficients, RNS context
    rns = _ctx(pkg, "rns", 4096, 2)
    many = [[int(x) for x in rng.integers(0, t, 6)] for _ in range(16)]
    cs = [int(x) for x in rng.integers(0, t, 16)]
    coms = [pkg.Commitment(rns, m, seed=200 + i) for i, m in enumerate(many)]
    comb = pkg.Commitment.linear_combine(rns, coms, cs)
    expect = [sum(decode_model.centred(c, t) * m[i] for c, m in zip(cs, many)) % t for i in range(6)]
    got, bits = comb.decode(rns, slots=6, noise=True)
    assert got.tolist() == expect and bits < rns.noise_capacity_bits
    full = comb.decode(rns)
    assert full.shape == (4096,) and full[:6].tolist() == expect and not full[6:].any()


_OTHER_PIPELINE = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as entry
pkg = entry.load_package()
for kind, name in (("default", "general"), ("rns", "rns-general")):
    params = pkg.Params(n=4096, k=2, sigma=3.19)
    ctx = pkg.LweContext.create_rns(params, key_seed=77) if kind == "rns" else pkg.LweContext(params, key_seed=77)
    assert ctx.pipeline == name, ctx.pipeline
    rows = np.load(sys.argv[2] + "/" + kind + "_rows.npy")
    msgs, status, bits = ctx.decode_rows(rows, noise=True)
    few = ctx.decode_rows(rows, slots=9)[0]
    np.savez(sys.argv[2] + "/" + kind + "_out.npz", msgs=msgs, status=status, bits=bits, few=few)
    ctx.close()
"""


def test_pipelines_agree(pkg, tmp_path):
    """64 rows (a few of them malformed) at (4096, 2), default and RNS: the single-launch pipelines against the general composition of
    a context created under LAMBDA_SNARK_COMMIT_FUSED=0 (read once at creation: a fresh child process)."""
    rng = np.random.default_rng(64)
    mine = {}
    for kind, name in (("default", "tile"), ("rns", "rns-tile")):
        ctx = _ctx(pkg, kind, 4096, 2)
        assert ctx.pipeline == name
        msgs = rng.integers(0, 2**64, size=(64, 4096), dtype=np.uint64)
        rows = _commit(ctx, msgs, 4096, rng.integers(1, 2**63, size=64, dtype=np.uint64))
        rows[:8] = _random_canonical_rows(ctx, rows[0], 8, rng)           # rows of every noise level
        rows[9, 1] ^= 1
        rows[11, 40] = 2**63
        np.save(str(tmp_path / (kind + "_rows.npy")), rows)
        mine[kind] = ctx.decode_rows(rows, noise=True) + (ctx.decode_rows(rows, slots=9)[0],)
    script = tmp_path / "other.py"
    script.write_text(_OTHER_PIPELINE)
    subprocess.run([sys.executable, str(script), ROOT, str(tmp_path)], check=True, env=dict(os.environ, LAMBDA_SNARK_COMMIT_FUSED="0"), timeout=600)
    for kind in ("default", "rns"):
        other = np.load(str(tmp_path / (kind + "_out.npz")))
        msgs, status, bits, few = mine[kind]
        assert status.tolist() == [1] * 9 + [-1, 1, -1] + [1] * 52 and np.array_equal(other["status"], status)
        good = status == 1                                                 # messages and noise of a malformed row are unspecified
        assert np.array_equal(other["msgs"][good], msgs[good]) and np.array_equal(other["few"][good], few[good])
        assert np.array_equal(other["bits"][good], bits[good])


@pytest.mark.parametrize("kind,n,k", [("default", 4096, 2), ("default", 1024, 3), ("default", 65536, 2), ("wide", 4096, 2), ("rns", 4096, 2), ("rns", 1024, 3)])
def test_malformed_rows(pkg, kind, n, k):
    ctx = _ctx(pkg, kind, n, k)
    other = _ctx(pkg, "default" if kind == "rns" else "rns", n, k)
    t = ctx.plain_modulus
    rng = np.random.default_rng(n + 3 * k)
    pair = ctx.rns_moduli()
    head, block = (6 if pair else 5), (k + 1) * n
    msgs = rng.integers(0, t, size=(11, 6), dtype=np.uint64)
    rows = _commit(ctx, msgs, 6, rng.integers(1, 2**63, size=11, dtype=np.uint64))
    clean = _decode_device(ctx, rows, 6)
    assert clean[1].tolist() == [1] * 11 and np.array_equal(clean[0], msgs)
    q_first, q_last = (pair or (ctx.commit_modulus,))[0], (pair or (ctx.commit_modulus,))[-1]
    rows[1, 1] ^= 1                                                  # magic
    rows[3, 2] = n | ((k + 1) << 32)                                 # n | k
    rows[5, head + 17] = q_first                                     # a word >= q in u
    rows[7, rows.shape[1] - 1] = q_last + 5                          # a word >= q in v (RNS: in v_2)
    rows[8, head + k * n + n - 1] = 2**63                            # ... and at the end of v (RNS: of v_1)
    foreign = _commit(other, msgs[:1], 6, [9])[0]                    # a row of the other kind of context, cut or padded to this row length
    rows[9, :] = 0
    width = min(rows.shape[1], foreign.size)
    rows[9, :width] = foreign[:width]
    bad = [1, 3, 5, 7, 8, 9]
    for slots in (6, n):
        got, status, bits = _decode_all(pkg, ctx, rows, slots)
        assert status.tolist() == [-1 if j in bad else 1 for j in range(11)]
        for j in range(11):
            if j not in bad:
                assert np.array_equal(got[j, :6], msgs[j]) and not got[j, 6:].any() and bits[j] == clean[2][j]


def test_fused_chunks_and_chunk_lanes(pkg):
    """n = 2^16, rank 2 decodes 128 rows per chunk on two chunk lanes: 260 rows are three chunks, the third reusing the first one's
    workspace slot.  Three distinct commitments repeated, one malformed row in each chunk."""
    ctx = _ctx(pkg, "default", 65536, 2)
    t = ctx.plain_modulus
    rng = np.random.default_rng(260)
    msgs = rng.integers(0, t, size=(3, 4), dtype=np.uint64)
    base = _commit(ctx, msgs, 4, [7, 8, 9])
    few, _, base_bits = _decode_device(ctx, base, 4)
    assert np.array_equal(few, msgs)
    pick = np.arange(260) % 3
    rows = base[pick]
    bad = [5, 130, 259]
    for j in bad:
        rows[j, ctx.commitment_words - 1 - j] = 2**63
    got, status, bits = _decode_device(ctx, rows, 4)
    assert status.tolist() == [-1 if j in bad else 1 for j in range(260)]
    good = status == 1
    assert np.array_equal(got[good], msgs[pick][good]) and np.array_equal(bits[good], base_bits[pick][good])


def test_fused_chunks_failing_verdicts_past_the_first_chunk(pkg):
    """The openings of the same 260 rows (three chunks on two chunk lanes, the third reusing slot 0): a malformed row and a wrongly
    claimed row in every chunk.  Each verdict, its bad mark and its claimed message sit at the chunk's offset into the batch."""
    ctx = _ctx(pkg, "default", 65536, 2)
    t = ctx.plain_modulus
    rng = np.random.default_rng(260)
    msgs = rng.integers(0, t, size=(3, 4), dtype=np.uint64)
    base = _commit(ctx, msgs, 4, [7, 8, 9])
    pick = np.arange(260) % 3
    rows, claimed = base[pick], msgs[pick]
    bad, wrong = [5, 130, 259], [7, 131, 258]
    for j in bad:
        rows[j, ctx.commitment_words - 1 - j] = 2**63
    for j in wrong:
        claimed[j, j % 4] = (claimed[j, j % 4] + 1) % t
    want = [-1 if j in bad else 0 if j in wrong else 1 for j in range(260)]
    assert _verify_device(ctx, rows, claimed) == want
    assert pkg.verify_openings_words(ctx, rows, claimed) == want


@pytest.mark.parametrize("n,k", [(4096, 2), (8192, 2)])
def test_decode_is_ordered_behind_a_commit_on_another_stream(pkg, n, k):
    """lsr_lwe_commit_rows_device on stream A, then lsr_lwe_decode_rows_device of those rows on stream B with no synchronisation by
    the caller: the context orders the two calls."""
    import torch
    ctx = _ctx(pkg, "default", n, k)
    rng = np.random.default_rng(11)
    batch, msg_len = 40, 5
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for it in range(6):
        msgs = rng.integers(0, ctx.plain_modulus, size=(batch, msg_len), dtype=np.uint64)
        keys = ctx.commit_keys(msgs, rng.integers(1, 2**63, size=batch, dtype=np.uint64))
        d_msgs, d_keys = torch.from_numpy(msgs.view(np.int64)).cuda(), torch.from_numpy(keys.view(np.int64)).cuda()
        d_rows = torch.zeros((batch, ctx.commitment_words), dtype=torch.int64, device="cuda")
        d_out = torch.full((batch, msg_len), -1, dtype=torch.int64, device="cuda")
        d_status = torch.zeros(batch, dtype=torch.int32, device="cuda")
        d_bits = torch.zeros(batch, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.commit_rows_device(d_msgs.data_ptr(), msg_len, batch, d_keys.data_ptr(), d_rows.data_ptr(), streams[0].cuda_stream)
        ctx.decode_rows_device(d_rows.data_ptr(), batch, msg_len, d_out.data_ptr(), d_status.data_ptr(), d_bits.data_ptr(), streams[1].cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(d_out.cpu().numpy().view(np.uint64), msgs), it
        assert d_status.cpu().tolist() == [1] * batch and int(d_bits.min().item()) > 0
