"""Fold of ring vectors by challenges under an arbitrary modulus: the fused lsr_ring_mod_fold_batch_device against the route composed
from the public pieces of the same handle, on the same seeded device-resident operands, in one process, the routes alternating after a
warm-up.  Prints ONE JSON line.

  new:        the fused call with the bounds of the row (0: none); where a row declares bound_p, `new_unbounded` is the same call
              without it (more groups of terms, the same words).
  route:      the composed route batch.h documents for a caller without the fused call: lsr_ring_mod_lift_batch_device of v and of p for
              each prime (four launches; two lifted copies of v exist in memory), then per group of at most max_terms terms two
              lsr_ntt_ring_fold_batch_device on the prime contexts and one lsr_ring_mod_reduce_batch_device (accumulating from the second
              group on).  A group's challenges must be contiguous per output, so the route reads p in group-major layout
              ([group][outputs][terms of the group][n]); that copy of p is prepared outside the timed region.
  floor:      (information) ONE lsr_ntt_ring_fold_batch_device on the first prime's context over all terms of the lifted operands: a
              fold at an NTT prime.  Two primes cost two of it and a reduce.

Shapes: the three of tools/ring_fold_bench.py that a handle admits, moved under q — (a) n = 4096, q = 2^32, 1024 outputs x 4 disjoint
terms x width 16; (l) n = 64, q = 4294967197 (the largest prime = 5 (mod 8) below 2^32) at the proportions of a LaBRADOR amortisation
step, 16 outputs x 32 disjoint terms x width 1024; (b) n = 4096, q = 2^32, 64 outputs over 256 shared terms x width 4 — and (g) n = 64,
q = 2^40 + 15, 64 outputs x width 64 with 9, 33 and 258 disjoint terms and challenges within 2: the route runs ceil(terms / 7) groups, the
call with bound_p = 2 one.
The outputs of the routes must be equal word for word before anything is timed.
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
Q41 = (1 << 40) + 15
# (label, n, q, outputs, terms, term_stride, width, bound_p or 0)
SHAPES = [("a", 4096, 1 << 32, 1024, 4, 4, 16, 0), ("l", 64, Q_5_MOD_8, 16, 32, 32, 1024, 0), ("b", 4096, 1 << 32, 64, 256, 0, 4, 0),
          ("g9", 64, Q41, 64, 9, 9, 64, 2), ("g33", 64, Q41, 64, 33, 33, 64, 2), ("g258", 64, Q41, 64, 258, 258, 64, 2)]


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


def measure(pkg, label, n, q, outputs, terms, stride, width, bound_p, reps, warmup):
    ring = pkg.RingMod(q, n, device=0)
    ctxs = [ring.prime_context(i) for i in range(2)]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(n + terms + width)
    s = torch.cuda.current_stream().cuda_stream
    vectors, vec = (outputs - 1) * stride + terms, width * n
    v = torch.randint(0, q, (vectors, width, n), dtype=torch.int64, device="cuda", generator=gen)
    if bound_p:
        p = torch.randint(-bound_p, bound_p + 1, (outputs, terms, n), dtype=torch.int64, device="cuda", generator=gen) % q
    else:
        p = torch.randint(0, q, (outputs, terms, n), dtype=torch.int64, device="cuda", generator=gen)
    # the route's groups of terms and its group-major copy of p
    group = min(terms, ring.max_terms)
    bounds = [(i0, min(i0 + group, terms)) for i0 in range(0, terms, group)]
    grouped = torch.empty(outputs * terms * n, dtype=torch.int64, device="cuda")
    offsets = [outputs * i0 * n for i0, _ in bounds]
    for (i0, i1), at in zip(bounds, offsets):
        grouped[at:at + outputs * (i1 - i0) * n].view(outputs, i1 - i0, n).copy_(p[:, i0:i1])
    lifted_v = [torch.empty_like(v) for _ in range(2)]
    lifted_p = [torch.empty_like(grouped) for _ in range(2)]
    res = [torch.empty((outputs, width, n), dtype=torch.int64, device="cuda") for _ in range(2)]
    outs = {name: torch.empty((outputs, width, n), dtype=torch.int64, device="cuda") for name in ("new", "new_unbounded", "route", "floor")}
    status = torch.zeros(outputs, dtype=torch.int32, device="cuda")
    floor_v, floor_p = torch.empty_like(v), torch.empty_like(p)
    ring.lift_device(0, floor_v.data_ptr(), v.data_ptr(), v.numel(), s)
    ring.lift_device(0, floor_p.data_ptr(), p.data_ptr(), p.numel(), s)

    def new():
        ring.fold_device(outs["new"].data_ptr(), status.data_ptr(), v.data_ptr(), p.data_ptr(), outputs, terms, stride, width, 0, bound_p, s)

    def new_unbounded():
        ring.fold_device(outs["new_unbounded"].data_ptr(), status.data_ptr(), v.data_ptr(), p.data_ptr(), outputs, terms, stride, width, 0, 0, s)

    def route():
        for i in range(2):
            ring.lift_device(i, lifted_v[i].data_ptr(), v.data_ptr(), v.numel(), s)
            ring.lift_device(i, lifted_p[i].data_ptr(), grouped.data_ptr(), grouped.numel(), s)
        for g, ((i0, i1), at) in enumerate(zip(bounds, offsets)):
            for i in range(2):
                ctxs[i].ring_fold_device(res[i].data_ptr(), lifted_v[i].data_ptr() + 8 * i0 * vec, lifted_p[i].data_ptr() + 8 * at, outputs, i1 - i0, stride,
                                         width, s)
            ring.reduce_device(outs["route"].data_ptr(), res[0].data_ptr(), res[1].data_ptr(), outputs * vec, g > 0, s)

    def floor():
        ctxs[0].ring_fold_device(outs["floor"].data_ptr(), floor_v.data_ptr(), floor_p.data_ptr(), outputs, terms, stride, width, s)

    routes = (("new", new),) + ((("new_unbounded", new_unbounded),) if bound_p else ()) + (("route", route), ("floor", floor))
    for _, fn in routes:
        fn()
    torch.cuda.synchronize()
    equal = bool(torch.equal(outs["new"], outs["route"])) and bool((status == 1).all())
    if bound_p:
        equal = equal and bool(torch.equal(outs["new_unbounded"], outs["route"]))
    half = q // 2
    row = {"shape": label, "n": n, "q": q, "outputs": outputs, "terms": terms, "term_stride": stride, "width": width, "bound_p": bound_p,
           "max_terms": ring.max_terms, "capacity_product": pkg.ring_mod_capacity_product(q, n, half, bound_p or half), "route_groups": len(bounds),
           "outputs_equal": equal}
    if not equal:
        raise SystemExit("ring_mod_fold_bench: the routes disagree on shape %s: %s" % (label, json.dumps(row)))
    row.update(timed(routes, reps, warmup))
    row["ratio_route_over_new"] = round(row["route"]["us_median"] / row["new"]["us_median"], 2)
    row["ratio_new_over_floor"] = round(row["new"]["us_median"] / row["floor"]["us_median"], 2)
    if bound_p:
        row["ratio_route_over_new_unbounded"] = round(row["route"]["us_median"] / row["new_unbounded"]["us_median"], 2)
    ring.close()
    return row


def main():
    reps, warmup = int(os.environ.get("REPS", "12")), int(os.environ.get("WARMUP", "2"))
    pkg = entry.load_package()
    rows = []
    for shape in SHAPES:
        rows.append(measure(pkg, *shape, reps, warmup))
        torch.cuda.empty_cache()
    out = {"tool": "ring_mod_fold_bench", "reps": reps, "warmup": warmup, "rows": rows, "all_equal": all(r["outputs_equal"] for r in rows),
           "provenance": provenance.provenance()}
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
