"""The twisted inner product of a ring handle under an arbitrary modulus, lsr_ring_mod_dot_galois_batch_device at g = 2n - 1, against
the two routes that existed without it, and two coefficient-wise calls on the handle's coefficient context beside the same calls on a
prime context — on seeded device-resident operands, in one process, the routes alternating after a warm-up.  Prints ONE JSON line.

  new:      lsr_ring_mod_dot_galois_batch_device.
  composed: (i) four lsr_ring_mod_lift_batch_device launches (a and b for each prime), two lsr_ntt_ring_dot_galois_batch_device on the
            handle's prime contexts and one lsr_ring_mod_reduce_batch_device (lifted operands and residues allocated outside the timing).
  twostep:  (ii) lsr_ntt_ring_automorphism_batch_device on the coefficient context, then lsr_ring_mod_dot_batch_device.
  floor:    the plain lsr_ring_mod_dot_batch_device on the same shape: what the call should cost if the permutation is free.
The yardsticks are composed, twostep and floor; the call under test is never its own.  A difference counts as a gain or a loss only
beyond the two spreads (max - min).  The outputs of new, composed and twostep must be equal word for word before anything is timed.

Shapes: n = 64, q = 4294967197, batch 16384, terms 16, with b per output and with a shared b; n = 4096, q = 2^32,
batch 1024, terms 4; n = 256, q = 3329, batch 65536, terms 1.

Also, at n = 64 with 16384 vectors of width 16: ring_l2sq and ring_scalar_combine (3 sets, 16 terms over 16384 / 16 outputs) on the
coefficient context of q = 4294967197 beside the same calls on prime_context(0) — the same kernels with another ModParams on the same
words (below both moduli; each context centres and reduces against its own modulus, so the outputs are not compared here: the tests
hold each to the integer models).
env REPS (default 12), WARMUP (2), OUT (a JSON file to write, with the provenance stamp)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import __graft_entry__ as entry  # noqa: E402
import provenance  # noqa: E402

Q_5_MOD_8 = 4294967197
SHAPES = [(64, Q_5_MOD_8, 16384, 16, False), (64, Q_5_MOD_8, 16384, 16, True), (4096, 1 << 32, 1024, 4, False), (256, 3329, 65536, 1, False)]


def timed(routes, reps, warmup):
    for _ in range(warmup):
        for _, fn in routes:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in routes}
    for _ in range(reps):
        for name, fn in routes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3)
    out = {}
    for name, _ in routes:
        t = times[name]
        out[name] = {"us_median": round(float(np.median(t)), 1), "us_min": round(float(np.min(t)), 1), "us_max": round(float(np.max(t)), 1),
                     "us_spread": round(float(np.max(t) - np.min(t)), 1)}
    return out


def verdict(out, new, other):
    """'gain' / 'loss' of `new` against `other` only beyond the two spreads, else 'within'"""
    a, b = out[new], out[other]
    margin = a["us_spread"] + b["us_spread"]
    if a["us_median"] + margin < b["us_median"]:
        return "gain"
    if b["us_median"] + margin < a["us_median"]:
        return "loss"
    return "within"


def measure_dot_galois(pkg, n, q, batch, terms, shared_b, reps, warmup):
    ring = pkg.RingMod(q, n, device=0)
    assert terms <= ring.max_terms
    ctxs, coeff = [ring.prime_context(i) for i in range(2)], ring.coeff_context()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(n + terms + shared_b)
    s = torch.cuda.current_stream().cuda_stream
    b_rows, g = (1 if shared_b else batch), 2 * n - 1
    a = torch.randint(0, q, (batch, terms, n), dtype=torch.int64, device="cuda", generator=gen)
    b = torch.randint(0, q, (b_rows, terms, n), dtype=torch.int64, device="cuda", generator=gen)
    outs = {name: torch.empty((batch, n), dtype=torch.int64, device="cuda") for name in ("new", "composed", "twostep", "floor")}
    la, lb = [torch.empty_like(a) for _ in range(2)], [torch.empty_like(b) for _ in range(2)]
    res = [torch.empty((batch, n), dtype=torch.int64, device="cuda") for _ in range(2)]
    sa = torch.empty_like(a)

    def new():
        ring.ring_dot_galois_device(outs["new"].data_ptr(), a.data_ptr(), b.data_ptr(), batch, terms, b_rows, g, s)

    def composed():
        for i in range(2):
            ring.lift_device(i, la[i].data_ptr(), a.data_ptr(), a.numel(), s)
            ring.lift_device(i, lb[i].data_ptr(), b.data_ptr(), b.numel(), s)
            ctxs[i].ring_dot_galois_device(res[i].data_ptr(), la[i].data_ptr(), lb[i].data_ptr(), batch, terms, b_rows, g, s)
        ring.reduce_device(outs["composed"].data_ptr(), res[0].data_ptr(), res[1].data_ptr(), batch * n, False, s)

    def twostep():
        coeff.ring_automorphism_device(sa.data_ptr(), a.data_ptr(), batch * terms, g, s)
        ring.dot_device(outs["twostep"].data_ptr(), sa.data_ptr(), b.data_ptr(), batch, terms, b_rows, s)

    def floor():
        ring.dot_device(outs["floor"].data_ptr(), a.data_ptr(), b.data_ptr(), batch, terms, b_rows, s)

    routes = (("new", new), ("composed", composed), ("twostep", twostep), ("floor", floor))
    for _, fn in routes:
        fn()
    torch.cuda.synchronize()
    row = {"op": "ring_mod_dot_galois", "n": n, "q": q, "g": g, "batch": batch, "terms": terms, "b_rows": b_rows, "max_terms": ring.max_terms,
           "outputs_equal": bool(torch.equal(outs["new"], outs["composed"]) and torch.equal(outs["new"], outs["twostep"]))}
    if row["outputs_equal"]:
        row.update(timed(routes, reps, warmup))
        row["against"] = {other: verdict(row, "new", other) for other in ("composed", "twostep", "floor")}
    ring.close()
    return row


def measure_coefficient_calls(pkg, reps, warmup):
    """ring_l2sq and ring_scalar_combine on the coefficient context of q = 4294967197 and on prime_context(0): operands below both moduli"""
    n, q, vectors, width, sets, terms = 64, Q_5_MOD_8, 16384, 16, 3, 16
    ring = pkg.RingMod(q, n, device=0)
    contexts = {"coeff": ring.coeff_context(), "prime": ring.prime_context(0)}
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    s = torch.cuda.current_stream().cuda_stream
    x = torch.randint(0, q, (vectors, width, n), dtype=torch.int64, device="cuda", generator=gen)
    count = vectors // terms
    weights = torch.randint(0, q, (1, sets, terms), dtype=torch.int64, device="cuda", generator=gen)
    rows = []

    norms = {name: torch.empty((vectors, 2), dtype=torch.int64, device="cuda") for name in contexts}
    routes = tuple((name, (lambda name=name, ctx=ctx: ctx.ring_l2sq_device(x.data_ptr(), vectors, width, norms[name].data_ptr(), s)))
                   for name, ctx in contexts.items())
    for _, fn in routes:
        fn()
    torch.cuda.synchronize()
    row = {"op": "ring_l2sq", "n": n, "q": q, "prime": ring.primes[0], "vectors": vectors, "width": width}      # (each centres against its own modulus)
    row.update(timed(routes, reps, warmup))
    row["against"] = {"prime": verdict(row, "coeff", "prime")}
    rows.append(row)

    outs = {name: torch.empty((count, sets, width, n), dtype=torch.int64, device="cuda") for name in contexts}
    status = torch.zeros((count,), dtype=torch.int32, device="cuda")
    routes = tuple((name, (lambda name=name, ctx=ctx: ctx.ring_scalar_combine_device(outs[name].data_ptr(), status.data_ptr(), x.data_ptr(),
                                                                                      weights.data_ptr(), 0, count, sets, terms, terms, width, count, s)))
                   for name, ctx in contexts.items())
    for _, fn in routes:
        fn()
    torch.cuda.synchronize()
    row = {"op": "ring_scalar_combine", "n": n, "q": q, "prime": ring.primes[0], "outputs": count, "sets": sets, "terms": terms, "width": width,
           "status_all_one": bool((status == 1).all())}
    row.update(timed(routes, reps, warmup))
    row["against"] = {"prime": verdict(row, "coeff", "prime")}
    rows.append(row)
    ring.close()
    return rows


def main():
    reps, warmup = int(os.environ.get("REPS", "12")), int(os.environ.get("WARMUP", "2"))
    pkg = entry.load_package()
    rows = []
    for n, q, batch, terms, shared_b in SHAPES:
        rows.append(measure_dot_galois(pkg, n, q, batch, terms, shared_b, reps, warmup))
        torch.cuda.empty_cache()
    rows += measure_coefficient_calls(pkg, reps, warmup)
    out = {"tool": "ring_mod_coeff_bench", "reps": reps, "warmup": warmup, "rows": rows,
           "all_equal": all(r.get("outputs_equal", True) for r in rows),
           "not_measured": ["host forms", "the integer flavour (lsr_set_arith_mode(1))", "n < 64"], "provenance": provenance.provenance()}
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
