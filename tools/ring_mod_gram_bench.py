"""Gram matrices of bounded ring vectors under an arbitrary modulus: lsr_ring_mod_gram_batch_device and
lsr_ring_mod_gram_sym2_batch_device against the route composed from the public pieces of the same handle, on the same seeded
device-resident operands, in one process, the routes alternating after a warm-up.  Prints ONE JSON line.

  new:     the call, with the bound of the shape (operands drawn within it).
  nobound: (shapes with a bound) the same call with both bounds "none": what stating the bound buys or costs.
  route:   the composed route of batch.h: lsr_ring_mod_lift_batch_device of a (and b) for each prime; then per group of max_terms
           columns (sym2: max_terms / 2) a strided copy of the group's columns into a dense [batch][r][group][n] buffer per prime —
           timed: the columns of a group are not contiguous across vectors; one group needs none — one
           lsr_ntt_ring_gram(_sym2)_batch_device on each lsr_ring_mod_prime_context and one lsr_ring_mod_reduce_batch_device,
           accumulating from the second group on.
  floor:   (information) ONE single-prime lsr_ntt_ring_gram(_sym2)_batch_device on the first prime's context over all columns.

Shapes: (A) n = 64, q = 4294967197, r = 16 symmetric, width 1024, batch 16, bound 128; (B) the same at q = 2^40 + 15, width 258 (the
route runs 37 groups, the call one); (C) n = 4096, q = 2^32, r = 16, width 16, batch 16, no bound; (D) sym2 at (C)'s shape; (E)
n = 256, q = 3329, r = 4, width 4, batch 4096.  The outputs of the routes must be equal word for word and every status 1.
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
# (label, n, q, r, width, batch, bound, sym2)
SHAPES = [("A", 64, Q_5_MOD_8, 16, 1024, 16, 128, False), ("B", 64, Q41, 16, 258, 16, 128, False), ("C", 4096, 1 << 32, 16, 16, 16, 0, False),
          ("D", 4096, 1 << 32, 16, 16, 16, 0, True), ("E", 256, 3329, 4, 4, 4096, 0, False)]


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


def draw(gen, q, shape, bound):
    if not bound:
        return torch.randint(0, q, shape, dtype=torch.int64, device="cuda", generator=gen)
    v = torch.randint(-bound, bound + 1, shape, dtype=torch.int64, device="cuda", generator=gen)
    return torch.where(v < 0, v + q, v)


def measure(pkg, label, n, q, r, width, batch, bound, sym2, reps, warmup):
    ring = pkg.RingMod(q, n, device=0)
    ring.gram_prepare()
    ctxs = [ring.prime_context(i) for i in range(2)]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(n + width + batch)
    s = torch.cuda.current_stream().cuda_stream
    pairs = r * (r + 1) // 2
    a = draw(gen, q, (batch, r, width, n), bound)
    b = draw(gen, q, (batch, r, width, n), bound) if sym2 else None
    operands = [a] + ([b] if sym2 else [])
    group = min(width, ring.max_terms // 2 if sym2 else ring.max_terms)
    bounds = [(c0, min(c0 + group, width)) for c0 in range(0, width, group)]
    lifted = [[torch.empty_like(x) for x in operands] for _ in range(2)]                       # [prime][operand]
    dense = [[torch.empty(batch * r * group * n, dtype=torch.int64, device="cuda") for _ in operands] for _ in range(2)] if len(bounds) > 1 else None
    res = [torch.empty((batch, pairs, n), dtype=torch.int64, device="cuda") for _ in range(2)]
    outs = {name: torch.full((batch, pairs, n), -1, dtype=torch.int64, device="cuda") for name in ("new", "nobound", "route", "floor")}
    status = {name: torch.zeros(batch, dtype=torch.int32, device="cuda") for name in ("new", "nobound")}

    def call(name, bnd):
        if sym2:
            ring.gram_sym2_device(outs[name].data_ptr(), status[name].data_ptr(), a.data_ptr(), b.data_ptr(), batch, r, width, bnd, bnd, s)
        else:
            ring.gram_device(outs[name].data_ptr(), status[name].data_ptr(), a.data_ptr(), None, batch, r, r, width, bnd, bnd, s)

    def single(ctx, out, ops, w):
        if sym2:
            ctx.ring_gram_sym2_device(out.data_ptr(), ops[0].data_ptr(), ops[1].data_ptr(), batch, r, w, s)
        else:
            ctx.ring_gram_device(out.data_ptr(), ops[0].data_ptr(), None, batch, r, r, w, s)

    def route():
        for i in range(2):
            for x, lx in zip(operands, lifted[i]):
                ring.lift_device(i, lx.data_ptr(), x.data_ptr(), x.numel(), s)
        for g, (c0, c1) in enumerate(bounds):
            for i in range(2):
                ops = lifted[i]
                if dense is not None:
                    ops = [d[:batch * r * (c1 - c0) * n].view(batch, r, c1 - c0, n) for d in dense[i]]
                    for d, lx in zip(ops, lifted[i]):
                        d.copy_(lx[:, :, c0:c1])
                single(ctxs[i], res[i], ops, c1 - c0)
            ring.reduce_device(outs["route"].data_ptr(), res[0].data_ptr(), res[1].data_ptr(), batch * pairs * n, g > 0, s)

    def floor():
        single(ctxs[0], outs["floor"], lifted[0], width)

    routes = (("new", lambda: call("new", bound)),) + ((("nobound", lambda: call("nobound", 0)),) if bound else ()) + (("route", route), ("floor", floor))
    for _, fn in routes:
        fn()
    torch.cuda.synchronize()
    h = q // 2
    row = {"shape": label, "op": "ring_mod_gram_sym2" if sym2 else "ring_mod_gram", "n": n, "q": q, "r": r, "width": width, "batch": batch, "bound": bound,
           "max_terms": ring.max_terms, "capacity_product": pkg.ring_mod_capacity_product(q, n, bound or h, bound or h), "route_groups": len(bounds),
           "outputs_equal": bool(torch.equal(outs["new"], outs["route"])) and (not bound or bool(torch.equal(outs["new"], outs["nobound"]))),
           "status_all_one": bool((status["new"] == 1).all())}
    row.update(timed(routes, reps, warmup))
    row["ratio_route_over_new"] = round(row["route"]["us_median"] / row["new"]["us_median"], 2)
    row["ratio_new_over_floor"] = round(row["new"]["us_median"] / row["floor"]["us_median"], 2)
    row["new_below_route_by_more_than_the_spreads"] = bool(row["route"]["us_median"] - row["new"]["us_median"] > row["route"]["us_spread"] + row["new"]["us_spread"])
    if bound:
        row["ratio_nobound_over_new"] = round(row["nobound"]["us_median"] / row["new"]["us_median"], 2)
    ring.close()
    return row


def main():
    reps, warmup = int(os.environ.get("REPS", "12")), int(os.environ.get("WARMUP", "2"))
    pkg = entry.load_package()
    rows = []
    for shape in SHAPES:
        rows.append(measure(pkg, *shape, reps, warmup))
        torch.cuda.empty_cache()
    out = {"tool": "ring_mod_gram_bench", "reps": reps, "warmup": warmup, "rows": rows,
           "all_equal": all(r["outputs_equal"] and r["status_all_one"] for r in rows), "provenance": provenance.provenance()}
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
