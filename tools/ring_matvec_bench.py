"""Ring matrix-vector product y_j = M x_j with a resident matrix (lsr_ntt_ring_matvec_batch_device) against the only route a caller had
before it, on the same seeded device-resident operands, in one process, the two routes alternating after a warm-up.  Prints ONE JSON
line.

  (route) per row r one lsr_ntt_ring_dot_batch_device with M[r] as the shared b (b_rows = 1) into a dense [batch][n] temporary, plus
          the strided copy into y[:, r].
The matrix handle is created outside the timed region (that is its point: M is transformed once, not per call); its creation time
is reported beside the timings.

Shapes, n = 4096 at q = 17592169062401: (a) rows 4, cols 16, batch 1024; (b) rows 64, cols 256, batch 3.
Criterion on (a): the new call's median + spread (max - min) below the route's median.  (b) is reported as measured.
Forward and inverse transforms per output vector: new cols * ceil(rows / row_block) + rows, route rows * cols + rows (plus the route's
rows * cols transforms of M per call).
env REPS (default 12), WARMUP (2), OUT (a JSON file to write, with the provenance stamp)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import __graft_entry__ as entry  # noqa: E402
import provenance  # noqa: E402

Q_TILE = 17592169062401
SHAPES = [("a", Q_TILE, 4096, 4, 16, 1024), ("b", Q_TILE, 4096, 64, 256, 3)]


def measure(pkg, name, q, n, rows, cols, batch, reps, warmup):
    ctx = pkg.NttContext(q, n, device=0)
    g = torch.Generator(device="cuda")
    g.manual_seed(n + rows + cols)
    s = torch.cuda.current_stream().cuda_stream
    m = torch.randint(0, q, (rows, cols, n), dtype=torch.int64, device="cuda", generator=g)
    x = torch.randint(0, q, (batch, cols, n), dtype=torch.int64, device="cuda", generator=g)
    y_new, y_route = (torch.empty((batch, rows, n), dtype=torch.int64, device="cuda") for _ in range(2))
    tmp = torch.empty((batch, n), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mat = ctx.ring_matrix_device(m.data_ptr(), rows, cols, s)
    torch.cuda.synchronize()
    create_us = (time.perf_counter() - t0) * 1e6
    b_rows = 1 if batch > 1 else batch

    def new():
        mat.matvec_device(y_new.data_ptr(), x.data_ptr(), batch, s)

    def route():
        for r in range(rows):
            ctx.ring_dot_device(tmp.data_ptr(), x.data_ptr(), m[r].data_ptr(), batch, cols, b_rows, s)
            y_route[:, r].copy_(tmp)

    new()
    route()
    torch.cuda.synchronize()
    equal = bool(torch.equal(y_new, y_route))
    routes = (("new", new), ("route", route))
    for _ in range(warmup):
        for _, fn in routes:
            fn()
    torch.cuda.synchronize()
    times = {key: [] for key, _ in routes}
    for _ in range(reps):
        for key, fn in routes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[key].append(e0.elapsed_time(e1) * 1e3)
    row_block = mat.row_block
    mat.close()
    ctx.close()
    row = {"shape": name, "n": n, "q": q, "rows": rows, "cols": cols, "batch": batch, "row_block": row_block, "outputs_equal": equal,
           "matrix_create_us": round(create_us, 1),
           "transforms_per_vector": {"new": cols * -(-rows // row_block) + rows, "route": rows * cols + rows}}
    for key, _ in routes:
        t = times[key]
        row[key] = {"us_median": round(float(np.median(t)), 1), "us_min": round(float(np.min(t)), 1), "us_max": round(float(np.max(t)), 1),
                    "us_spread": round(float(np.max(t) - np.min(t)), 1)}
    row["ratio_route_over_new"] = round(row["route"]["us_median"] / row["new"]["us_median"], 2)
    row["new_median_plus_spread_below_route_median"] = bool(row["new"]["us_median"] + row["new"]["us_spread"] < row["route"]["us_median"])
    return row


def main():
    reps, warmup = int(os.environ.get("REPS", "12")), int(os.environ.get("WARMUP", "2"))
    pkg = entry.load_package()
    rows = []
    for shape in SHAPES:
        rows.append(measure(pkg, *shape, reps, warmup))
        torch.cuda.empty_cache()
    out = {"tool": "ring_matvec_bench", "reps": reps, "warmup": warmup, "shapes": rows, "all_equal": all(r["outputs_equal"] for r in rows),
           "criterion_met_on_a": rows[0]["new_median_plus_spread_below_route_median"], "provenance": provenance.provenance()}
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
