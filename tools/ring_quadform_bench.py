"""The ring quadratic form of a packed symmetric matrix (lsr_ntt_ring_quadform_batch_device) against the route it
replaces, and the symmetrised packed Gram matrix (lsr_ntt_ring_gram_sym2_batch_device) against the cross Gram matrix packed in torch.
One process, seeded device-resident operands, the routes alternating after a warm-up, outputs compared word for word at every shape.
Prints ONE JSON line.

  quadform   new  one ring_quadform_device (challenges per family, offdiag = 2).
             R1   the composed route end to end: a torch gather of the factors of every pair product c_i c_l, one ring_mul_device,
                  the scaling of the off-diagonal products by offdiag mod q in torch, one ring_dot_device with terms = pairs.
             R2   the same with the gather OUTSIDE the timed region (products and scaling stay inside: they depend on the fresh c).
  sym2       new  one ring_gram_sym2_device.
             X    the cross form of ring_gram_device (all r^2 outputs), then x_il + x_li mod q packed in torch.
  (A) n = 64, r = 16, batch 16        (B) n = 4096, r = 16, batch 16        (C) n = 65536, r = 8, batch 4
  (D) n = 4096, r = 2, batch 1024 (little to share);  sym2 width: 16, at (C) 4.
Criterion: at (A) and (B) the quadratic form's median lies below R1's by more than the sum of the two spreads (R2 is reported beside it).

The kernels alone: `kernel_model` computes, from the shape, the bytes the pointwise kernel must move (every g-hat and c-hat word read
once, every output word written once) and the bytes its loads request (a g-hat word and a c-hat_l word per pair, c-hat_i once per
row; the pieces of rows that slices share add to it and are not counted).  Per-kernel times come from a kernel trace taken in a run
of its own:
  SHAPES=A CALLS=quadform NEW_ONLY=1 rocprofv3 --kernel-trace --stats --output-format csv -- python tools/ring_quadform_bench.py
and are merged with KERNEL_STATS=A:<stats csv>,B:<stats csv>; NEW_ONLY runs make 1 + WARMUP + REPS calls.

env REPS (default 12), WARMUP (2), OUT (a JSON file to write, with the provenance stamp), SHAPES (default ABCD), CALLS (default
quadform,sym2), NEW_ONLY=1, KERNEL_STATS (above), LIBVARIANT (an experiment build of the library, csrc/Makefile VARIANT=...; use with
NEW_ONLY=1)."""
import csv
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import __graft_entry__ as entry  # noqa: E402
import provenance  # noqa: E402
from ring_gram_bench import timed  # noqa: E402

Q12, Q16 = 17592169062401, 17592180539393        # the FP64 flavour up to n = 4096 and at n = 2^16
# name: (n, q, r, batch, width of sym2)
SHAPES = {"A": (64, Q12, 16, 16, 16), "B": (4096, Q12, 16, 16, 16), "C": (65536, Q16, 8, 4, 4), "D": (4096, Q12, 2, 1024, 16)}
OFFDIAG = 2


def triangle(r):
    return [(i, l) for i in range(r) for l in range(i, r)]


def kernel_model(n, r, batch):
    """Counts per call of the quadratic form, from the shape alone."""
    pairs = r * (r + 1) // 2
    return {"pairs": pairs,
            "bytes_must_move": 8 * n * batch * (pairs + r + 1),
            "bytes_loads_request": 8 * n * batch * (pairs + (pairs - r) + r),
            "products_done": n * batch * (pairs + 2 * r), "products_of_a_product_per_pair": n * batch * 2 * pairs,
            "forward_transforms": batch * (r + pairs), "inverse_transforms": batch,
            "route_forward_transforms": batch * 4 * pairs, "route_inverse_transforms": batch * (pairs + 1)}


def kernel_times_us(path, calls):
    """{kernel: [us per call, launches per call]} of a `rocprofv3 --kernel-trace --stats` CSV of a NEW_ONLY run over one shape and call."""
    with open(path) as f:
        rows = list(csv.DictReader(f))
    out = {}
    for r in rows:
        short = re.sub(r"[<(].*$", "", r["Name"].replace("void ", "").replace("(anonymous namespace)::", "")).split("::")[-1]
        us, launches = out.get(short, (0.0, 0.0))
        out[short] = (us + int(r["TotalDurationNs"]) / 1e3 / calls, launches + int(r["Calls"]) / calls)
    return {k: [round(v[0], 2), round(v[1], 2)] for k, v in sorted(out.items(), key=lambda kv: -kv[1][0])}


def finish(row, routes, reps, warmup, reference):
    row.update(timed(routes, reps, warmup))
    for other in [name for name, _ in routes if name != "new"]:
        row["ratio_%s_over_new" % other] = round(row[other]["us_median"] / row["new"]["us_median"], 2)
    for ref in reference.split(","):
        if ref in row:
            row["new_below_%s_by_more_than_both_spreads" % ref] = bool(
                row[ref]["us_median"] - row["new"]["us_median"] > row[ref]["us_spread"] + row["new"]["us_spread"])
    return row


def measure_quadform(pkg, name, reps, warmup, new_only, stats):
    n, q, r, batch, _ = SHAPES[name]
    ctx = pkg.NttContext(q, n, device=0)
    s = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda")
    gen.manual_seed(ord(name))
    idx = triangle(r)
    pairs = len(idx)
    g = torch.randint(0, q, (batch, pairs, n), dtype=torch.int64, device="cuda", generator=gen)
    c = torch.randint(0, q, (batch, r, n), dtype=torch.int64, device="cuda", generator=gen)
    out_new = torch.empty((batch, n), dtype=torch.int64, device="cuda")

    def new():
        ctx.ring_quadform_device(out_new.data_ptr(), g.data_ptr(), c.data_ptr(), batch, r, batch, OFFDIAG, s)

    routes = [("new", new)]
    if not new_only:
        ii = torch.tensor([i for i, _ in idx], device="cuda")
        ll = torch.tensor([l for _, l in idx], device="cuda")
        scale = torch.tensor([1 if i == l else OFFDIAG for i, l in idx], dtype=torch.int64, device="cuda")[None, :, None]
        out_r1, out_r2 = torch.empty_like(out_new), torch.empty_like(out_new)
        prod = torch.empty((batch, pairs, n), dtype=torch.int64, device="cuda")

        def composed(out, left, right):
            ctx.ring_mul_device(prod.data_ptr(), left.data_ptr(), right.data_ptr(), batch * pairs, batch * pairs, s)
            scaled = prod * scale % q                                  # (offdiag q < 2^63)
            ctx.ring_dot_device(out.data_ptr(), g.data_ptr(), scaled.data_ptr(), batch, pairs, batch, s)

        def r1():
            composed(out_r1, c.index_select(1, ii), c.index_select(1, ll))

        left_fixed, right_fixed = c.index_select(1, ii), c.index_select(1, ll)

        def r2():
            composed(out_r2, left_fixed, right_fixed)

        routes += [("R1", r1), ("R2", r2)]
    for _, fn in routes:
        fn()
    torch.cuda.synchronize()
    row = {"call": "quadform", "shape": name, "n": n, "q": q, "r": r, "batch": batch, "c_rows": batch, "offdiag": OFFDIAG,
           "temporary_bytes_of_the_route": 8 * n * batch * pairs, "kernel_model": kernel_model(n, r, batch)}
    if not new_only:
        row["outputs_equal"] = bool(torch.equal(out_new, out_r1) and torch.equal(out_new, out_r2))
    finish(row, routes, reps, warmup, "R1,R2")
    key = name + "q"
    if key in stats:
        row["kernels_alone_us_and_launches_per_call"] = kernel_times_us(stats[key], 1 + warmup + reps)
        us = sum(v[0] for k, v in row["kernels_alone_us_and_launches_per_call"].items() if k.startswith("ring_quadform"))
        m = row["kernel_model"]
        row["pointwise_kernels"] = {"us_per_call": round(us, 2), "TBps_of_bytes_must_move": round(m["bytes_must_move"] / us / 1e6, 3),
                                    "TBps_of_bytes_loads_request": round(m["bytes_loads_request"] / us / 1e6, 3)}
    ctx.close()
    return row


def measure_sym2(pkg, name, reps, warmup, new_only, stats):
    n, q, r, batch, width = SHAPES[name]
    ctx = pkg.NttContext(q, n, device=0)
    s = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda")
    gen.manual_seed(ord(name) + 1)
    idx = triangle(r)
    pairs = len(idx)
    a = torch.randint(0, q, (batch, r, width, n), dtype=torch.int64, device="cuda", generator=gen)
    b = torch.randint(0, q, (batch, r, width, n), dtype=torch.int64, device="cuda", generator=gen)
    h_new = torch.empty((batch, pairs, n), dtype=torch.int64, device="cuda")

    def new():
        ctx.ring_gram_sym2_device(h_new.data_ptr(), a.data_ptr(), b.data_ptr(), batch, r, width, s)

    routes = [("new", new)]
    if not new_only:
        ii = torch.tensor([i for i, _ in idx], device="cuda")
        ll = torch.tensor([l for _, l in idx], device="cuda")
        diagonal = (ii == ll)[None, :, None]
        x = torch.empty((batch, r, r, n), dtype=torch.int64, device="cuda")
        held = {}

        def cross():
            ctx.ring_gram_device(x.data_ptr(), a.data_ptr(), b.data_ptr(), batch, r, r, width, s)
            up, down = x[:, ii, ll], x[:, ll, ii]
            held["h"] = torch.where(diagonal, up, (up + down) % q)

        routes += [("X", cross)]
    for _, fn in routes:
        fn()
    torch.cuda.synchronize()
    row = {"call": "sym2", "shape": name, "n": n, "q": q, "r": r, "batch": batch, "width": width, "block_edge": ctx.ring_gram_block}
    if not new_only:
        row["outputs_equal"] = bool(torch.equal(h_new, held["h"]))
    finish(row, routes, reps, warmup, "X")
    key = name + "s"
    if key in stats:
        row["kernels_alone_us_and_launches_per_call"] = kernel_times_us(stats[key], 1 + warmup + reps)
    ctx.close()
    return row


def main():
    reps, warmup = int(os.environ.get("REPS", "12")), int(os.environ.get("WARMUP", "2"))
    new_only = os.environ.get("NEW_ONLY") == "1"
    calls = os.environ.get("CALLS", "quadform,sym2").split(",")
    # KERNEL_STATS=Aq:<csv of the quadratic form at (A)>,As:<csv of sym2 at (A)>, ...
    stats = dict(item.split(":", 1) for item in os.environ.get("KERNEL_STATS", "").split(",") if item)
    pkg = entry.load_package()
    variant = os.environ.get("LIBVARIANT")
    if variant:
        pkg._abi.use_library(os.path.join(os.path.dirname(pkg._abi.LIB_PATH), "liblambda_snark_core_%s.so" % variant))
    rows = []
    for name in os.environ.get("SHAPES", "ABCD"):
        if "quadform" in calls:
            rows.append(measure_quadform(pkg, name, reps, warmup, new_only, stats))
        if "sym2" in calls:
            rows.append(measure_sym2(pkg, name, reps, warmup, new_only, stats))
        torch.cuda.empty_cache()
    out = {"tool": "ring_quadform_bench", "library_variant": variant, "reps": reps, "warmup": warmup, "new_only": new_only, "rows": rows,
           "all_equal": all(r.get("outputs_equal", True) for r in rows),
           "criterion_met": {r["shape"]: r.get("new_below_R1_by_more_than_both_spreads") for r in rows if r["call"] == "quadform" and r["shape"] in "AB"},
           "provenance": provenance.provenance()}
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
