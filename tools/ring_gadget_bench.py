"""The fused commitment y = M G^-1(x) (lsr_ntt_ring_matvec_gadget_batch_device) against the only other route, on the same seeded
device-resident operands, in one process, the routes alternating after a warm-up.  Prints ONE JSON line.

  (route) lsr_ntt_ring_decompose_batch_device into a [batch][cols][n] temporary, then lsr_ntt_ring_matvec_batch_device on it;
  (floor) lsr_ntt_ring_matvec_batch_device alone on the pre-decomposed input: the same transforms as the fused call without the digit
          extraction and without the decomposition pass — what the fused call cannot be expected to beat by much.
The matrix handle is created outside the timed region.

Shapes, n = 4096 at q = 17592169062401: (a) rows 4, b = 11, D = 5, xcols 4 (cols 20), batch 1024; (b) rows 64, b = 4, D = 12,
xcols 21 (cols 252), batch 3.  Criterion on (a): the fused call's median + spread (max - min) below the route's median.  (b) is
reported as measured.  Reported beside them: the bytes of the route's temporary, and decompose alone as achieved bytes per second over
(1 + D) * 8 * n * count bytes (count = batch * xcols).
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

Q_TILE = 17592169062401
SHAPES = [("a", Q_TILE, 4096, 4, 11, 5, 4, 1024), ("b", Q_TILE, 4096, 64, 4, 12, 21, 3)]


def measure(pkg, name, q, n, rows, b, digits, xcols, batch, reps, warmup):
    assert pkg.ring_gadget_min_digits(q, b) == digits
    cols, count = xcols * digits, batch * xcols
    ctx = pkg.NttContext(q, n, device=0)
    g = torch.Generator(device="cuda")
    g.manual_seed(n + rows + cols)
    s = torch.cuda.current_stream().cuda_stream
    m = torch.randint(0, q, (rows, cols, n), dtype=torch.int64, device="cuda", generator=g)
    x = torch.randint(0, q, (batch, xcols, n), dtype=torch.int64, device="cuda", generator=g)
    y_fused, y_route, y_floor = (torch.empty((batch, rows, n), dtype=torch.int64, device="cuda") for _ in range(3))
    tmp = torch.empty((batch, cols, n), dtype=torch.int64, device="cuda")        # the route's temporary: D times the witness
    pre = torch.empty_like(tmp)
    mat = ctx.ring_matrix_device(m.data_ptr(), rows, cols, s)
    ctx.ring_decompose_device(pre.data_ptr(), x.data_ptr(), count, b, digits, s)

    def fused():
        mat.matvec_gadget_device(y_fused.data_ptr(), x.data_ptr(), batch, b, digits, s)

    def decompose():
        ctx.ring_decompose_device(tmp.data_ptr(), x.data_ptr(), count, b, digits, s)

    def route():
        decompose()
        mat.matvec_device(y_route.data_ptr(), tmp.data_ptr(), batch, s)

    def floor():
        mat.matvec_device(y_floor.data_ptr(), pre.data_ptr(), batch, s)

    routes = (("fused", fused), ("route", route), ("floor", floor), ("decompose", decompose))
    for _, fn in routes:
        fn()
    torch.cuda.synchronize()
    equal = bool(torch.equal(y_fused, y_route)) and bool(torch.equal(y_fused, y_floor))
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
    row = {"shape": name, "n": n, "q": q, "rows": rows, "base_log2": b, "digits": digits, "xcols": xcols, "cols": cols, "batch": batch,
           "row_block": row_block, "outputs_equal": equal, "route_temporary_bytes": batch * cols * n * 8, "witness_bytes": batch * xcols * n * 8}
    for key, _ in routes:
        t = times[key]
        row[key] = {"us_median": round(float(np.median(t)), 1), "us_min": round(float(np.min(t)), 1), "us_max": round(float(np.max(t)), 1),
                    "us_spread": round(float(np.max(t) - np.min(t)), 1)}
    decompose_bytes = (1 + digits) * 8 * n * count
    row["decompose"]["bytes"] = decompose_bytes
    row["decompose"]["gb_per_s"] = round(decompose_bytes / row["decompose"]["us_median"] / 1e3, 1)
    row["ratio_route_over_fused"] = round(row["route"]["us_median"] / row["fused"]["us_median"], 2)
    row["ratio_fused_over_floor"] = round(row["fused"]["us_median"] / row["floor"]["us_median"], 2)
    row["fused_median_plus_spread_below_route_median"] = bool(row["fused"]["us_median"] + row["fused"]["us_spread"] < row["route"]["us_median"])
    return row


def main():
    reps, warmup = int(os.environ.get("REPS", "12")), int(os.environ.get("WARMUP", "2"))
    pkg = entry.load_package()
    rows = []
    for shape in SHAPES:
        rows.append(measure(pkg, *shape, reps, warmup))
        torch.cuda.empty_cache()
    out = {"tool": "ring_gadget_bench", "reps": reps, "warmup": warmup, "shapes": rows, "all_equal": all(r["outputs_equal"] for r in rows),
           "criterion_met_on_a": rows[0]["fused_median_plus_spread_below_route_median"], "provenance": provenance.provenance()}
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
