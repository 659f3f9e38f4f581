"""The batched ring Gram matrix G = A B^T (lsr_ntt_ring_gram_batch_device) against the route it replaces: one
lsr_ntt_ring_dot_batch_device over every pair on gathered operands.  One process, seeded device-resident operands, the routes
alternating after a warm-up, outputs compared word for word.  Prints ONE JSON line.

  R1  the route end to end: a torch gather of both operands into [batch * pairs][width][n], then one ring_dot_device.
  R2  the route's best case: the same ring_dot_device on operands gathered OUTSIDE the timed region.
  (A) n = 4096, width 16, r = 16 symmetric, batch 16        (B) n = 4096, width 16, cross ra = rb = 16, batch 8
  (C) n = 65536, width 4, r = 8 symmetric, batch 4          (D) n = 4096, width 16, r = 2 symmetric, batch 1024 (the call saves least)
Criterion: at (A) and (B) the new call's median lies below R2's by more than the sum of the two spreads.

The Gram kernel alone: `kernel_model` computes, from the shape, the bytes the kernel must move (every operand word read once, every
output word written once), the loads it issues (E + E words per column, position and block pair) and the modular products it must do
and does (a diagonal block of the symmetric form computes all E x E).  Its time comes from a kernel trace taken in a run of its own:
  SHAPES=A NEW_ONLY=1 rocprofv3 --kernel-trace --stats --output-format csv -- python tools/ring_gram_bench.py
and is merged with KERNEL_STATS=A:<stats csv>,B:<stats csv>; NEW_ONLY runs make 1 + WARMUP + REPS calls.

env REPS (default 12), WARMUP (2), OUT (a JSON file to write, with the provenance stamp), SHAPES (default ABCD), NEW_ONLY=1,
KERNEL_STATS (above), LIBVARIANT (an experiment build of the library, csrc/Makefile VARIANT=...; use with NEW_ONLY=1)."""
import csv
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

Q12, Q16 = 17592169062401, 17592180539393        # the FP64 flavour at n = 4096 and at n = 2^16
# name: (n, q, width, ra, rb (0: symmetric), batch)
SHAPES = {"A": (4096, Q12, 16, 16, 0, 16), "B": (4096, Q12, 16, 16, 16, 8), "C": (65536, Q16, 4, 8, 0, 4), "D": (4096, Q12, 16, 2, 0, 1024)}
# MI355X peaks the kernel's rates are set against: HBM3E 8 TB/s; 256 CUs x 4 SIMDs x 16 FP64 lanes x 2.4 GHz vector FP64 instructions,
# 7 of them per product of the FP64 flavour (mulmod_f64: mul, fma, mul, rint, fma, add; one add into the accumulator)
HBM_BYTES_PER_S = 8.0e12
F64_PRODUCTS_PER_S = 256 * 4 * 16 * 2.4e9 / 7


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


def pair_indices(ra, rb):
    """(i, l) of every output in stored order; rb == 0: the packed upper triangle"""
    return [(i, l) for i in range(ra) for l in range(i if rb == 0 else 0, rb or ra)]


def kernel_model(n, width, ra, rb, batch, edge):
    """Counts per call, from the shape alone."""
    sym = rb == 0
    bi, bl = -(-ra // edge), -(-(rb or ra) // edge)
    block_pairs = bi * (bi + 1) // 2 if sym else bi * bl
    outs = len(pair_indices(ra, rb))
    vectors = ra if sym else ra + rb
    return {"outputs": outs * batch, "block_pairs": block_pairs,
            "bytes_must_move": 8 * n * batch * (vectors * width + outs),
            "bytes_loaded": 8 * n * batch * block_pairs * 2 * edge * width,
            "products_must_do": n * batch * outs * width,
            "products_done": n * batch * block_pairs * edge * edge * width,
            "forward_transforms": batch * vectors * width, "inverse_transforms": batch * outs,
            "route_forward_transforms": 2 * batch * outs * width}


def kernel_time_us(path, calls):
    """Total time of ring_gram_kernel in a `rocprofv3 --kernel-trace --stats` CSV of a NEW_ONLY run over one shape, per call."""
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if "ring_gram_kernel" in r["Name"]]
    if not rows:
        raise SystemExit("no ring_gram_kernel row in " + path)
    return sum(int(r["TotalDurationNs"]) for r in rows) / 1e3 / calls, sum(int(r["Calls"]) for r in rows) / calls


def measure(pkg, name, reps, warmup, new_only, stats):
    n, q, width, ra, rb, batch = SHAPES[name]
    ctx = pkg.NttContext(q, n, device=0)
    s = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda")
    gen.manual_seed(ord(name))
    a = torch.randint(0, q, (batch, ra, width, n), dtype=torch.int64, device="cuda", generator=gen)
    b = torch.randint(0, q, (batch, rb, width, n), dtype=torch.int64, device="cuda", generator=gen) if rb else None
    idx = pair_indices(ra, rb)
    pairs = len(idx)
    ii = torch.tensor([i for i, _ in idx], device="cuda")
    ll = torch.tensor([l for _, l in idx], device="cuda")
    g_new = torch.empty((batch, pairs, n), dtype=torch.int64, device="cuda")

    def new():
        ctx.ring_gram_device(g_new.data_ptr(), a.data_ptr(), b.data_ptr() if rb else 0, batch, ra, rb or ra, width, s)

    routes = [("new", new)]
    if not new_only:
        g_r1, g_r2 = torch.empty_like(g_new), torch.empty_like(g_new)
        right = b if rb else a

        def r1():
            u = a.index_select(1, ii)
            v = right.index_select(1, ll)
            ctx.ring_dot_device(g_r1.data_ptr(), u.data_ptr(), v.data_ptr(), batch * pairs, width, batch * pairs, s)

        u_fixed, v_fixed = a.index_select(1, ii), right.index_select(1, ll)

        def r2():
            ctx.ring_dot_device(g_r2.data_ptr(), u_fixed.data_ptr(), v_fixed.data_ptr(), batch * pairs, width, batch * pairs, s)

        routes += [("R1", r1), ("R2", r2)]
    for _, fn in routes:
        fn()
    torch.cuda.synchronize()
    edge = ctx.ring_gram_block
    row = {"shape": name, "n": n, "q": q, "width": width, "ra": ra, "rb": rb or ra, "symmetric": rb == 0, "batch": batch, "block_edge": edge,
           "gathered_bytes_per_operand": 8 * n * width * batch * pairs, "kernel_model": kernel_model(n, width, ra, rb, batch, edge)}
    if not new_only:
        row["outputs_equal"] = bool(torch.equal(g_new, g_r1) and torch.equal(g_new, g_r2))
    row.update(timed(routes, reps, warmup))
    for other in ("R1", "R2"):
        if other in row:
            row["ratio_%s_over_new" % other] = round(row[other]["us_median"] / row["new"]["us_median"], 2)
    if "R2" in row:
        row["new_below_R2_by_more_than_both_spreads"] = bool(
            row["R2"]["us_median"] - row["new"]["us_median"] > row["R2"]["us_spread"] + row["new"]["us_spread"])
    if name in stats:
        us, launches = kernel_time_us(stats[name], 1 + warmup + reps)
        m = row["kernel_model"]
        frac_hbm = m["bytes_must_move"] / (us * 1e-6) / HBM_BYTES_PER_S
        frac_f64 = m["products_done"] / (us * 1e-6) / F64_PRODUCTS_PER_S
        row["kernel_alone"] = {"us_per_call": round(us, 1), "launches_per_call": launches, "stats_file": os.path.basename(stats[name]),
                               "TBps_of_bytes_must_move": round(m["bytes_must_move"] / us / 1e6, 2),
                               "TBps_of_bytes_loaded": round(m["bytes_loaded"] / us / 1e6, 2),
                               "G_products_done_per_s": round(m["products_done"] / us / 1e3, 1),
                               "fraction_of_hbm_peak": round(frac_hbm, 3), "fraction_of_f64_product_peak": round(frac_f64, 3),
                               "nearer_bound": "fp64 issue" if frac_f64 > frac_hbm else "hbm"}
    ctx.close()
    del a, b, g_new
    torch.cuda.empty_cache()
    return row


def main():
    reps, warmup = int(os.environ.get("REPS", "12")), int(os.environ.get("WARMUP", "2"))
    new_only = os.environ.get("NEW_ONLY") == "1"
    stats = dict(item.split(":", 1) for item in os.environ.get("KERNEL_STATS", "").split(",") if item)
    pkg = entry.load_package()
    variant = os.environ.get("LIBVARIANT")
    if variant:
        pkg._abi.use_library(os.path.join(os.path.dirname(pkg._abi.LIB_PATH), "liblambda_snark_core_%s.so" % variant))
    rows = [measure(pkg, name, reps, warmup, new_only, stats) for name in os.environ.get("SHAPES", "ABCD")]
    out = {"tool": "ring_gram_bench", "library_variant": variant, "reps": reps, "warmup": warmup, "new_only": new_only, "rows": rows,
           "all_equal": all(r.get("outputs_equal", True) for r in rows),
           "criterion_met": {r["shape"]: r.get("new_below_R2_by_more_than_both_spreads") for r in rows if r["shape"] in "AB"},
           "provenance": provenance.provenance()}
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
