"""Fused fold of ring vectors out[j][c] = sum_i p[j][i] v[j term_stride + i][c] (lsr_ntt_ring_fold_batch_device) against the route a
caller had before it, on the same seeded device-resident operands, in one process, the two routes alternating after a warm-up.  Prints
ONE JSON line.

  route: a torch gather of v into [outputs * width][terms][n], the challenges repeated `width` times into the same shape (both inside
         the timed region: they are what the caller has to do per fold), then lsr_ntt_ring_dot_batch_device with b_rows = batch.

Shapes: (a) n = 4096, 1024 outputs x 4 disjoint terms x width 16; (b) n = 4096, 64 outputs over 256 shared terms x width 4 (both at
q = 17592169062401); (c) n = 2^16, 64 outputs x 4 disjoint terms x width 4 at q = 17592180539393.
Criterion, on (a) only: the new call's median + spread (max - min) below the route's median.  (b) and (c) are reported as measured.
Transforms per output polynomial: new = terms + 1 + terms / width, route = 2 terms + 1.
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
# (label, q, n, outputs, terms, term_stride, width)
SHAPES = [("a", Q_TILE, 4096, 1024, 4, 4, 16), ("b", Q_TILE, 4096, 64, 256, 0, 4), ("c", Q_TWO_PASS, 65536, 64, 4, 4, 4)]


def measure(pkg, label, q, n, outputs, terms, stride, width, reps, warmup):
    ctx = pkg.NttContext(q, n, device=0)
    g = torch.Generator(device="cuda")
    g.manual_seed(n + terms + width)
    s = torch.cuda.current_stream().cuda_stream
    vectors = (outputs - 1) * stride + terms
    v = torch.randint(0, q, (vectors, width, n), dtype=torch.int64, device="cuda", generator=g)
    p = torch.randint(0, q, (outputs, terms, n), dtype=torch.int64, device="cuda", generator=g)
    rows = (torch.arange(outputs, device="cuda")[:, None] * stride + torch.arange(terms, device="cuda")[None, :])      # [outputs][terms]
    batch = outputs * width
    out_new = torch.empty((outputs, width, n), dtype=torch.int64, device="cuda")
    out_route = torch.empty_like(out_new)
    ga = torch.empty((outputs, width, terms, n), dtype=torch.int64, device="cuda")      # the route's two temporaries
    gb = torch.empty_like(ga)

    def new():
        ctx.ring_fold_device(out_new.data_ptr(), v.data_ptr(), p.data_ptr(), outputs, terms, stride, width, s)

    def route():
        ga.copy_(v[rows].transpose(1, 2))                           # [outputs][terms][width][n] -> [outputs][width][terms][n]
        gb.copy_(p[:, None].expand(outputs, width, terms, n))
        ctx.ring_dot_device(out_route.data_ptr(), ga.data_ptr(), gb.data_ptr(), batch, terms, batch, s)

    new()
    route()
    torch.cuda.synchronize()
    equal = bool(torch.equal(out_new, out_route))
    routes = (("new", new), ("route", route))
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
    row = {"shape": label, "n": n, "q": q, "outputs": outputs, "terms": terms, "term_stride": stride, "width": width, "outputs_equal": equal,
           "transforms_per_output_polynomial": {"new": round(terms + 1 + terms / width, 2), "route": 2 * terms + 1}}
    for name, _ in routes:
        t = times[name]
        row[name] = {"us_median": round(float(np.median(t)), 1), "us_min": round(float(np.min(t)), 1), "us_max": round(float(np.max(t)), 1),
                     "us_spread": round(float(np.max(t) - np.min(t)), 1)}
    row["ratio_route_over_new"] = round(row["route"]["us_median"] / row["new"]["us_median"], 2)
    if label == "a":
        row["criterion_met"] = bool(row["new"]["us_median"] + row["new"]["us_spread"] < row["route"]["us_median"])
    return row


def main():
    reps, warmup = int(os.environ.get("REPS", "12")), int(os.environ.get("WARMUP", "2"))
    pkg = entry.load_package()
    rows = []
    for shape in SHAPES:
        rows.append(measure(pkg, *shape, reps, warmup))
        torch.cuda.empty_cache()
    out = {"tool": "ring_fold_bench", "reps": reps, "warmup": warmup, "shapes": rows, "all_equal": all(r["outputs_equal"] for r in rows),
           "criterion_met": rows[0]["criterion_met"], "provenance": provenance.provenance()}
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
