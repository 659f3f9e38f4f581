"""Ring inner products under an arbitrary modulus: the fused lsr_ring_mod_dot_batch_device against the route composed from the
public pieces of the same handle — four lsr_ring_mod_lift_batch_device launches (a and b for each prime), two
lsr_ntt_ring_dot_batch_device on the handle's prime contexts and one lsr_ring_mod_reduce_batch_device — on the same seeded
device-resident operands, in one process, the routes alternating after a warm-up.  Prints ONE JSON line.

  new:      lsr_ring_mod_dot_batch_device.
  route:    the composed route above (its four lifted operands and two residue arrays are allocated outside the timed region).
  floor:    (information) ONE ordinary lsr_ntt_ring_dot_batch_device on the first prime's context over the same shapes: a ring inner
            product at an NTT prime.  Two primes should cost about twice it.

Shapes: n = 64, q = 4294967197 (the largest prime = 5 (mod 8) below 2^32), batch 16384, terms 16, with b per output and with a shared
b; n = 4096, q = 2^32, batch 1024, terms 4; n = 256, q = 3329, batch 65536, terms 1.
Criterion, per row: the new call's median + spread (max - min) below the route's median.  The outputs of the two routes must be equal
word for word.
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
    out["ratio_route_over_new"] = round(out["route"]["us_median"] / out["new"]["us_median"], 2)
    out["ratio_new_over_floor"] = round(out["new"]["us_median"] / out["floor"]["us_median"], 2)
    out["criterion_met"] = bool(out["new"]["us_median"] + out["new"]["us_spread"] < out["route"]["us_median"])
    return out


def measure(pkg, n, q, batch, terms, shared_b, reps, warmup):
    ring = pkg.RingMod(q, n, device=0)
    assert terms <= ring.max_terms
    ctxs = [ring.prime_context(i) for i in range(2)]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(n + terms + shared_b)
    s = torch.cuda.current_stream().cuda_stream
    b_rows = 1 if shared_b else batch
    a = torch.randint(0, q, (batch, terms, n), dtype=torch.int64, device="cuda", generator=gen)
    b = torch.randint(0, q, (b_rows, terms, n), dtype=torch.int64, device="cuda", generator=gen)
    outs = {name: torch.empty((batch, n), dtype=torch.int64, device="cuda") for name in ("new", "route", "floor")}
    la, lb = [torch.empty_like(a) for _ in range(2)], [torch.empty_like(b) for _ in range(2)]
    res = [torch.empty((batch, n), dtype=torch.int64, device="cuda") for _ in range(2)]

    def new():
        ring.dot_device(outs["new"].data_ptr(), a.data_ptr(), b.data_ptr(), batch, terms, b_rows, s)

    def route():
        for i in range(2):
            ring.lift_device(i, la[i].data_ptr(), a.data_ptr(), a.numel(), s)
            ring.lift_device(i, lb[i].data_ptr(), b.data_ptr(), b.numel(), s)
            ctxs[i].ring_dot_device(res[i].data_ptr(), la[i].data_ptr(), lb[i].data_ptr(), batch, terms, b_rows, s)
        ring.reduce_device(outs["route"].data_ptr(), res[0].data_ptr(), res[1].data_ptr(), batch * n, False, s)

    def floor():
        ctxs[0].ring_dot_device(outs["floor"].data_ptr(), a.data_ptr(), b.data_ptr(), batch, terms, b_rows, s)

    routes = (("new", new), ("route", route), ("floor", floor))
    for _, fn in routes:
        fn()
    torch.cuda.synchronize()
    row = {"op": "ring_mod_dot", "n": n, "q": q, "batch": batch, "terms": terms, "b_rows": b_rows, "max_terms": ring.max_terms,
           "outputs_equal": bool(torch.equal(outs["new"], outs["route"]))}
    row.update(timed(routes, reps, warmup))
    ring.close()
    return row


def main():
    reps, warmup = int(os.environ.get("REPS", "12")), int(os.environ.get("WARMUP", "2"))
    pkg = entry.load_package()
    rows = []
    for n, q, batch, terms, shared_b in SHAPES:
        rows.append(measure(pkg, n, q, batch, terms, shared_b, reps, warmup))
        torch.cuda.empty_cache()
    out = {"tool": "ring_mod_bench", "reps": reps, "warmup": warmup, "rows": rows, "all_equal": all(r["outputs_equal"] for r in rows),
           "criterion_met": all(r["criterion_met"] for r in rows), "provenance": provenance.provenance()}
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
