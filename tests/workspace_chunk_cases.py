"""The n > 4096 calls of tests/test_workspace_chunks_gpu.py whose device form walks the batch in chunks of a workspace sized from
LAMBDA_SNARK_NTT_CHUNK_MIB, each on inputs it builds from a fixed seed: the test runs a case in its own process under the default size
(256 MiB: one chunk) and in a fresh child under LAMBDA_SNARK_NTT_CHUNK_MIB=1, and compares every array.

At 1 MiB ring_mul_enqueue's chunk (lsr_ring_mul.hip) is 8 polynomials at n = 8192 and 1 at n = 2^17; matvec_composed's chunk
(lsr_ring_matvec.hip) and the rows of the inner product's workspace (lsr_ring_workspace.hpp) are 5 at n = 8192.  Each case states its
split and has three chunks with a ragged last one where the chunk is above 1.  The operands stay in INPUTS for the reference checks of
the test's own process; the child never reads it."""
import numpy as np

Q44 = 17592180539393           # 44-bit NTT prime, 2^18 | q - 1: every n up to 2^17 (FP64 kernels)
Q60 = 1152921504606584833      # 60-bit NTT prime (u64 Shoup kernels)
GOLD = 18446744069414584321    # CyclicNtt's modulus (Goldilocks kernels)

MUL_N, MUL_BATCH = 8192, 19
FIVE_STAGE_N, FIVE_STAGE_BATCH = 131072, 3
MATVEC_N, MATVEC_ROWS, MATVEC_COLS, MATVEC_BATCH = 8192, 2, 7, 12

INPUTS = {}                    # case name -> {key: operands} of the case's last run in this process


def _record(case, key, **operands):
    INPUTS.setdefault(case, {})[key] = operands


def _rand(rng, q, shape):
    return rng.integers(0, q, size=shape, dtype=np.uint64)


def _contexts(pkg, n, flavours):
    """(name, context, q) for each flavour: "f64" (Q44), "u64" (Q60) on NTT-friendly primes, "gold" the cyclic Goldilocks ring"""
    for flavour in flavours:
        if flavour == "gold":
            yield flavour, pkg.CyclicNtt(n), GOLD
        else:
            q = Q44 if flavour == "f64" else Q60
            ctx = pkg.NttContext(q, n, device=0)
            assert ctx.uses_f64 == (flavour == "f64")
            yield flavour, ctx, q


def _dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _mul_device(ctx, a, b, c_is=None):
    """a b through ring_mul_device: b [batch][n] or one shared row [n]; c_is: None (c apart from both operands), "a" or "b" (c is that
    operand's buffer)"""
    import torch
    d_a, d_b = _dev(torch, a), _dev(torch, b)
    d_c = {None: torch.full_like(d_a, -1), "a": d_a, "b": d_b}[c_is]
    ctx.ring_mul_device(d_c.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), a.shape[0], 1 if b.ndim == 1 else b.shape[0], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return _host(d_c)


def _ring_mul_two_pass(pkg, flavour):
    """n = 8192: chunk 8, batch 19 = 8 + 8 + 3.  Host form (one staging chunk: the device call below it walks the 19): b per product
    and shared.  Device form: c apart from both operands; c is a (the strided round in place); c is b (b goes into the workspace
    before c is written); a shared b, whose transform sits behind the chunk in the workspace, with c is a."""
    out, rng = {}, np.random.default_rng(31 + len(flavour))
    for name, ctx, q in _contexts(pkg, MUL_N, (flavour,)):
        a, b = _rand(rng, q, (MUL_BATCH, MUL_N)), _rand(rng, q, (MUL_BATCH, MUL_N))
        out["host each"], out["host shared"] = ctx.ring_mul(a, b), ctx.ring_mul(a, b[3])
        out["device apart"] = _mul_device(ctx, a, b)
        out["device c is a"], out["device c is b"] = _mul_device(ctx, a, b, "a"), _mul_device(ctx, a, b, "b")
        out["device shared c is a"] = _mul_device(ctx, a, b[3], "a")
        _record("ring_mul_two_pass_" + name, name, q=q, a=a, b=b, omega=ctx.omega if name == "gold" else 0)
        ctx.close()
    return out


def ring_mul_two_pass_f64(pkg):
    """_ring_mul_two_pass on the 44-bit prime (FP64 kernels)"""
    return _ring_mul_two_pass(pkg, "f64")


def ring_mul_two_pass_u64(pkg):
    """_ring_mul_two_pass on the 60-bit prime (u64 Shoup kernels)"""
    return _ring_mul_two_pass(pkg, "u64")


def ring_mul_two_pass_gold(pkg):
    """_ring_mul_two_pass on the cyclic Goldilocks ring"""
    return _ring_mul_two_pass(pkg, "gold")


def ring_mul_five_stage(pkg):
    """n = 2^17 (the five-stage strided round): chunk 1, batch 3 = 1 + 1 + 1, device form, b per product and shared (its transform
    behind a one-polynomial chunk)"""
    rng = np.random.default_rng(32)
    ctx = pkg.NttContext(Q44, FIVE_STAGE_N, device=0)
    a, b = _rand(rng, Q44, (FIVE_STAGE_BATCH, FIVE_STAGE_N)), _rand(rng, Q44, (FIVE_STAGE_BATCH, FIVE_STAGE_N))
    out = {"each": _mul_device(ctx, a, b), "shared": _mul_device(ctx, a, b[1])}
    _record("ring_mul_five_stage", "f64", q=Q44, a=a, b=b)
    ctx.close()
    return out


def matvec_composed(pkg):
    """a 2 x 7 matrix at n = 8192: chunk 5, batch 12 = 5 + 5 + 2, and inside every chunk the 7 columns of the shared matrix row go
    through the inner product's 5-polynomial workspace in two term groups (5 + 2); host and device form"""
    import torch
    out, rng = {}, np.random.default_rng(33)
    for name, ctx, q in _contexts(pkg, MATVEC_N, ("f64", "u64")):
        m, x = _rand(rng, q, (MATVEC_ROWS, MATVEC_COLS, MATVEC_N)), _rand(rng, q, (MATVEC_BATCH, MATVEC_COLS, MATVEC_N))
        with ctx.ring_matrix(m) as mat:
            out[name + " host"] = mat.matvec(x)
            d_x = _dev(torch, x)
            d_y = torch.full((MATVEC_BATCH, MATVEC_ROWS, MATVEC_N), -1, dtype=torch.int64, device="cuda")
            mat.matvec_device(d_y.data_ptr(), d_x.data_ptr(), MATVEC_BATCH, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            out[name + " device"] = _host(d_y)
        _record("matvec_composed", name, q=q, m=m, x=x)
        ctx.close()
    return out


CASES = {f.__name__: f for f in (ring_mul_two_pass_f64, ring_mul_two_pass_u64, ring_mul_two_pass_gold, ring_mul_five_stage, matvec_composed)}
