"""Ring quadratic forms under an arbitrary modulus: lsr_ring_mod_quadform_batch_device against the two routes a caller had before it,
on the same seeded device-resident operands, in one process, the routes alternating after a warm-up.  Prints ONE JSON line.

  new:    the call, offdiag 2, the challenges drawn and declared within 2, g unbounded.
  public: (n <= 4096) the route of the public API: a gather of (c_i, c_l) for every packed pair, ONE lsr_ring_mod_mul_batch_device over
          batch * pairs products, the off-diagonal products scaled by offdiag mod q (torch), ONE lsr_ring_mod_dot_batch_device with
          terms = pairs.  The gather and the scaling are timed: the route cannot do without them.  Above n = 4096 the fused mul and dot
          are refused and the route does not exist.
  pieces: lsr_ring_mod_lift_batch_device of g and of c for each prime (four lifts), lsr_ntt_ring_quadform_batch_device on each
          lsr_ring_mod_prime_context with offdiag's residue, one lsr_ring_mod_reduce_batch_device.  No exactness statement of the
          library covers this route; with the challenges within 2 it is exact (lsr_ring_mod_capacity_quadform), which is why it is
          comparable here.
  floor:  (information) ONE single-prime lsr_ntt_ring_quadform_batch_device on the first prime's context over lifted operands.

Shapes, all offdiag 2 and bound_c 2: (A) n = 64, q = 4294967197, r = 16, batch 16; (B) n = 4096, q = 2^32, r = 16, batch 16; (C)
n = 65536, q = 2^32, r = 8, batch 4; (D) n = 256, q = 3329, r = 2, batch 4096; (E) (A) with one shared c.  The outputs of the routes
must be equal word for word and every status 1 before anything is timed.
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
OFFDIAG, BOUND_C = 2, 2
# (label, n, q, r, batch, shared c)
SHAPES = [("A", 64, Q_5_MOD_8, 16, 16, False), ("B", 4096, 1 << 32, 16, 16, False), ("C", 65536, 1 << 32, 8, 4, False), ("D", 256, 3329, 2, 4096, False),
          ("E", 64, Q_5_MOD_8, 16, 16, True)]


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


def measure(pkg, label, n, q, r, batch, shared, reps, warmup):
    ring = pkg.RingMod(q, n, device=0)
    ring.gram_prepare()
    ctxs = [ring.prime_context(i) for i in range(2)]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(37 * n + r + batch)
    s = torch.cuda.current_stream().cuda_stream
    pairs, c_rows = r * (r + 1) // 2, 1 if shared else batch
    g = torch.randint(0, q, (batch, pairs, n), dtype=torch.int64, device="cuda", generator=gen)
    v = torch.randint(-BOUND_C, BOUND_C + 1, (c_rows, r, n), dtype=torch.int64, device="cuda", generator=gen)
    c = torch.where(v < 0, v + q, v)
    names = ("new", "pieces", "floor") + (("public",) if n <= 4096 else ())
    outs = {name: torch.full((batch, n), -1, dtype=torch.int64, device="cuda") for name in names}
    status = torch.zeros(batch, dtype=torch.int32, device="cuda")
    lifted_g = [torch.empty_like(g) for _ in range(2)]
    lifted_c = [torch.empty_like(c) for _ in range(2)]
    res = [torch.empty((batch, n), dtype=torch.int64, device="cuda") for _ in range(2)]
    order = [(i, l) for i in range(r) for l in range(i, r)]
    rows_i = torch.tensor([i for i, _ in order], device="cuda")
    rows_l = torch.tensor([l for _, l in order], device="cuda")
    scale = torch.tensor([1 if i == l else OFFDIAG for i, l in order], dtype=torch.int64, device="cuda")[None, :, None]
    products = torch.empty((batch, pairs, n), dtype=torch.int64, device="cuda") if n <= 4096 else None

    def new():
        ring.quadform_device(outs["new"].data_ptr(), status.data_ptr(), g.data_ptr(), c.data_ptr(), batch, r, c_rows, OFFDIAG, 0, BOUND_C, s)

    def public():
        ci, cl = c[:, rows_i].contiguous(), c[:, rows_l].contiguous()                          # [c_rows][pairs][n]
        count = c_rows * pairs
        ring.mul_device(products.data_ptr(), ci.data_ptr(), cl.data_ptr(), count, count, s)
        scaled = (products[:c_rows] * scale) % q
        ring.dot_device(outs["public"].data_ptr(), g.data_ptr(), scaled.data_ptr(), batch, pairs, c_rows, s)

    def pieces():
        for i in range(2):
            ring.lift_device(i, lifted_g[i].data_ptr(), g.data_ptr(), g.numel(), s)
            ring.lift_device(i, lifted_c[i].data_ptr(), c.data_ptr(), c.numel(), s)
            ctxs[i].ring_quadform_device(res[i].data_ptr(), lifted_g[i].data_ptr(), lifted_c[i].data_ptr(), batch, r, c_rows, OFFDIAG, s)
        ring.reduce_device(outs["pieces"].data_ptr(), res[0].data_ptr(), res[1].data_ptr(), batch * n, False, s)

    def floor():
        ctxs[0].ring_quadform_device(outs["floor"].data_ptr(), lifted_g[0].data_ptr(), lifted_c[0].data_ptr(), batch, r, c_rows, OFFDIAG, s)

    routes = (("new", new),) + ((("public", public),) if n <= 4096 else ()) + (("pieces", pieces), ("floor", floor))
    for _, fn in routes:
        fn()
    torch.cuda.synchronize()
    equal = bool(torch.equal(outs["new"], outs["pieces"])) and (n > 4096 or bool(torch.equal(outs["new"], outs["public"])))
    row = {"shape": label, "op": "ring_mod_quadform", "n": n, "q": q, "r": r, "pairs": pairs, "batch": batch, "c_rows": c_rows, "offdiag": OFFDIAG,
           "bound_c": BOUND_C, "capacity_quadform": pkg.ring_mod_capacity_quadform(q, n, 0, BOUND_C), "outputs_equal": equal,
           "outputs_nonzero": bool(outs["new"].any()), "status_all_one": bool((status == 1).all())}
    if not (row["outputs_equal"] and row["status_all_one"]):
        ring.close()
        return row                                             # nothing is timed before the routes agree
    row.update(timed(routes, reps, warmup))
    row["ratio_pieces_over_new"] = round(row["pieces"]["us_median"] / row["new"]["us_median"], 2)
    row["ratio_new_over_floor"] = round(row["new"]["us_median"] / row["floor"]["us_median"], 2)
    if n <= 4096:
        row["ratio_public_over_new"] = round(row["public"]["us_median"] / row["new"]["us_median"], 2)
        row["new_below_public_by_more_than_the_spreads"] = bool(
            row["public"]["us_median"] - row["new"]["us_median"] > row["public"]["us_spread"] + row["new"]["us_spread"])
    ring.close()
    return row


def main():
    reps, warmup = int(os.environ.get("REPS", "12")), int(os.environ.get("WARMUP", "2"))
    pkg = entry.load_package()
    rows = []
    for shape in SHAPES:
        rows.append(measure(pkg, *shape, reps, warmup))
        torch.cuda.empty_cache()
    out = {"tool": "ring_mod_quadform_bench", "reps": reps, "warmup": warmup, "rows": rows,
           "all_equal": all(r["outputs_equal"] and r["status_all_one"] for r in rows), "provenance": provenance.provenance()}
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))
    return 0 if out["all_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
