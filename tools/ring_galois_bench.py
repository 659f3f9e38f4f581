"""Galois automorphisms out = sigma_g(x) (lsr_ntt_ring_automorphism_batch_device) and the twisted ring inner product
c = sum_i sigma_g(a_i) b_i (lsr_ntt_ring_dot_galois_batch_device) against the route a caller had before them, on the same seeded
device-resident operands, in one process, the routes alternating after a warm-up.  Prints ONE JSON line.

  route:    a torch index_select on the last axis and a masked q - x (the index and the sign mask of g are the caller's constants and
            built outside the timed region; the gather, the negation and the temporary they need are inside it); for the inner
            product followed by lsr_ntt_ring_dot_batch_device.
  composed: (inner product only, information) lsr_ntt_ring_automorphism_batch_device + lsr_ntt_ring_dot_batch_device.

Shapes, each at g = 2 n - 1 and g = 5: automorphism at n = 4096 x 16384 polynomials (q = 17592169062401) and at n = 2^16 x 1024
polynomials (q = 17592180539393); inner product at n = 4096, batch 1024, terms 4 with b per output and with a shared b.
Criterion, per row: the new call's median + spread (max - min) below the route's median.  The automorphism rows also carry the
achieved bytes/s against the 16 bytes a word the operation has to move.
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

Q_TILE, Q_TWO_PASS = 17592169062401, 17592180539393


def gather_constants(n, g):
    """(source index, negated?) of output word j on a negacyclic context: s = j g^-1 mod 2 n."""
    s = (torch.arange(n, dtype=torch.int64, device="cuda") * pow(g, -1, 2 * n)) % (2 * n)
    return (s % n).contiguous(), (s >= n).contiguous()


def torch_automorphism(x, q, idx, neg):
    y = x.index_select(-1, idx)
    return torch.where(neg & (y != 0), q - y, y)


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
    out["ratio_route_over_new"] = round(out["route"]["us_median"] / out["new"]["us_median"], 2)
    out["criterion_met"] = bool(out["new"]["us_median"] + out["new"]["us_spread"] < out["route"]["us_median"])
    return out


def measure_automorphism(pkg, q, n, count, g, reps, warmup):
    ctx = pkg.NttContext(q, n, device=0)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(n + g)
    s = torch.cuda.current_stream().cuda_stream
    x = torch.randint(0, q, (count, n), dtype=torch.int64, device="cuda", generator=gen)
    out_new, out_route = torch.empty_like(x), torch.empty_like(x)
    idx, neg = gather_constants(n, g)

    def new():
        ctx.ring_automorphism_device(out_new.data_ptr(), x.data_ptr(), count, g, s)

    def route():
        out_route.copy_(torch_automorphism(x, q, idx, neg))

    new()
    route()
    torch.cuda.synchronize()
    row = {"op": "automorphism", "n": n, "q": q, "count": count, "g": g, "outputs_equal": bool(torch.equal(out_new, out_route))}
    row.update(timed((("new", new), ("route", route)), reps, warmup))
    row["new_algorithmic_GBps"] = round(16.0 * count * n / row["new"]["us_median"] / 1e3, 1)
    ctx.close()
    return row


def measure_dot(pkg, q, n, batch, terms, shared_b, g, reps, warmup):
    ctx = pkg.NttContext(q, n, device=0)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(n + g + terms + shared_b)
    s = torch.cuda.current_stream().cuda_stream
    b_rows = 1 if shared_b else batch
    a = torch.randint(0, q, (batch, terms, n), dtype=torch.int64, device="cuda", generator=gen)
    b = torch.randint(0, q, (b_rows, terms, n), dtype=torch.int64, device="cuda", generator=gen)
    outs = {name: torch.empty((batch, n), dtype=torch.int64, device="cuda") for name in ("new", "route", "composed")}
    sa_route, sa_composed = torch.empty_like(a), torch.empty_like(a)      # the temporaries of the two other routes
    idx, neg = gather_constants(n, g)

    def new():
        ctx.ring_dot_galois_device(outs["new"].data_ptr(), a.data_ptr(), b.data_ptr(), batch, terms, b_rows, g, s)

    def route():
        sa_route.copy_(torch_automorphism(a, q, idx, neg))
        ctx.ring_dot_device(outs["route"].data_ptr(), sa_route.data_ptr(), b.data_ptr(), batch, terms, b_rows, s)

    def composed():
        ctx.ring_automorphism_device(sa_composed.data_ptr(), a.data_ptr(), batch * terms, g, s)
        ctx.ring_dot_device(outs["composed"].data_ptr(), sa_composed.data_ptr(), b.data_ptr(), batch, terms, b_rows, s)

    routes = (("new", new), ("route", route), ("composed", composed))
    for _, fn in routes:
        fn()
    torch.cuda.synchronize()
    row = {"op": "dot_galois", "n": n, "q": q, "batch": batch, "terms": terms, "b_rows": b_rows, "g": g,
           "outputs_equal": bool(torch.equal(outs["new"], outs["route"]) and torch.equal(outs["new"], outs["composed"]))}
    row.update(timed(routes, reps, warmup))
    row["ratio_composed_over_new"] = round(row["composed"]["us_median"] / row["new"]["us_median"], 2)
    ctx.close()
    return row


def main():
    reps, warmup = int(os.environ.get("REPS", "12")), int(os.environ.get("WARMUP", "2"))
    pkg = entry.load_package()
    rows = []
    for q, n, count in [(Q_TILE, 4096, 16384), (Q_TWO_PASS, 65536, 1024)]:
        for g in (2 * n - 1, 5):
            rows.append(measure_automorphism(pkg, q, n, count, g, reps, warmup))
            torch.cuda.empty_cache()
    for shared_b in (False, True):
        for g in (2 * 4096 - 1, 5):
            rows.append(measure_dot(pkg, Q_TILE, 4096, 1024, 4, shared_b, g, reps, warmup))
            torch.cuda.empty_cache()
    out = {"tool": "ring_galois_bench", "reps": reps, "warmup": warmup, "rows": rows, "all_equal": all(r["outputs_equal"] for r in rows),
           "criterion_met": all(r["criterion_met"] for r in rows), "provenance": provenance.provenance()}
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
