"""Fused ring inner product c_j = sum_i a_{j,i} b_{j,i} (lsr_ntt_ring_dot_batch_device) against the two routes a caller had before it, on
the same seeded device-resident operands, in one process, the three routes alternating after a warm-up.  Prints ONE JSON line.

  (A) `terms` calls of lsr_ntt_ring_mul_batch_device into a temporary, each followed by a torch addition mod q;
  (B) lsr_ntt_forward_batch_device on all operands, lsr_ntt_mul_pointwise_device per term, an int64 torch accumulation reduced mod q,
      one lsr_ntt_inverse_batch_device.
Both routes get their operands term-major ([terms][batch][n], prepared outside the timed region), which is what their per-term calls
need.  Route (B)'s transforms work in place: the equality check runs it on fresh copies; the timed repetitions transform the same
buffers again (a transform costs the same on any canonical input), so no copy is charged to it.  With a shared b, (B) transforms b
once and repeats each b-hat row over the batch for the pointwise call, which takes [count] operands.

Shapes: n = 4096 at q = 17592169062401, terms in {2, 4, 16} with batch * terms = 32768, per-output b and shared b; n = 2^16 at
q = 17592182243329, terms = 4, batch 512.  Criterion: the new call's median + spread (max - min) below (B)'s median.
Algorithmic bytes per output residue: 16 terms + 8 (8 terms + 8 with a shared b); the fraction is of 8 TB/s.
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

HBM_BYTES_PER_S = 8.0e12
Q_TILE, Q_TWO_PASS = 17592169062401, 17592182243329
SHAPES = [(Q_TILE, 4096, 2, 16384), (Q_TILE, 4096, 4, 8192), (Q_TILE, 4096, 16, 2048), (Q_TWO_PASS, 65536, 4, 512)]


def measure(pkg, q, n, terms, batch, shared, reps, warmup):
    ctx = pkg.NttContext(q, n, device=0)
    g = torch.Generator(device="cuda")
    g.manual_seed(n + terms)
    s = torch.cuda.current_stream().cuda_stream
    b_rows = 1 if shared else batch
    a = torch.randint(0, q, (batch, terms, n), dtype=torch.int64, device="cuda", generator=g)
    b = torch.randint(0, q, (b_rows, terms, n), dtype=torch.int64, device="cuda", generator=g)
    a_t, b_t = a.transpose(0, 1).contiguous(), b.transpose(0, 1).contiguous()      # [terms][batch | 1][n]
    ta, tb = torch.empty_like(a_t), torch.empty_like(b_t)
    c_new, c_a, c_b = (torch.empty((batch, n), dtype=torch.int64, device="cuda") for _ in range(3))
    tmp = torch.empty_like(c_new)
    rep = torch.empty_like(c_new) if shared else None

    def new():
        ctx.ring_dot_device(c_new.data_ptr(), a.data_ptr(), b.data_ptr(), batch, terms, b_rows, s)

    def route_a():
        for i in range(terms):
            ctx.ring_mul_device((c_a if i == 0 else tmp).data_ptr(), a_t[i].data_ptr(), b_t[i].data_ptr(), batch, b_rows, s)
            if i:
                c_a.add_(tmp)
                c_a.remainder_(q)

    def route_b():
        ctx.forward_device(ta.data_ptr(), terms * batch, s)
        ctx.forward_device(tb.data_ptr(), terms * b_rows, s)
        for i in range(terms):
            if shared:
                rep.copy_(tb[i].expand(batch, n))
            ctx.mul_pointwise_device((c_b if i == 0 else tmp).data_ptr(), ta[i].data_ptr(), (rep if shared else tb[i]).data_ptr(), batch * n, s)
            if i:
                c_b.add_(tmp)
                c_b.remainder_(q)
        ctx.inverse_device(c_b.data_ptr(), batch, s)

    ta.copy_(a_t)
    tb.copy_(b_t)
    new()
    route_a()
    route_b()
    torch.cuda.synchronize()
    equal = bool(torch.equal(c_new, c_a)) and bool(torch.equal(c_new, c_b))
    routes = (("new", new), ("A", route_a), ("B", route_b))
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
    ctx.close()
    per_residue = (8 if shared else 16) * terms + 8
    row = {"n": n, "q": q, "terms": terms, "batch": batch, "b_rows": b_rows, "outputs_equal": equal, "algorithmic_bytes_per_residue": per_residue}
    for name, _ in routes:
        t = times[name]
        row[name] = {"us_median": round(float(np.median(t)), 1), "us_min": round(float(np.min(t)), 1), "us_max": round(float(np.max(t)), 1),
                     "us_spread": round(float(np.max(t) - np.min(t)), 1)}
    us = row["new"]["us_median"]
    row["ratio_A_over_new"] = round(row["A"]["us_median"] / us, 2)
    row["ratio_B_over_new"] = round(row["B"]["us_median"] / us, 2)
    row["fraction_of_8TBps"] = round(per_residue * batch * n / (us * 1e-6) / HBM_BYTES_PER_S, 3)
    row["criterion_met"] = bool(us + row["new"]["us_spread"] < row["B"]["us_median"])
    return row


def main():
    reps, warmup = int(os.environ.get("REPS", "12")), int(os.environ.get("WARMUP", "2"))
    pkg = entry.load_package()
    rows = []
    for q, n, terms, batch in SHAPES:
        for shared in ((False, True) if n == 4096 else (False,)):
            rows.append(measure(pkg, q, n, terms, batch, shared, reps, warmup))
            torch.cuda.empty_cache()
    out = {"tool": "ring_dot_bench", "reps": reps, "warmup": warmup, "shapes": rows, "all_equal": all(r["outputs_equal"] for r in rows),
           "criterion_met_everywhere": all(r["criterion_met"] for r in rows), "provenance": provenance.provenance()}
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
