"""The scalar-weighted aggregation of ring vectors (lsr_ntt_ring_scalar_combine_batch_device) against the only route the
library had for it: ring_fold with every scalar dressed up as a constant polynomial.  One process, seeded device-resident operands,
the routes alternating after a warm-up, the outputs compared word for word at every shape.  Prints ONE JSON line.

  new:  the fused device call without an addend.
  new+: the fused device call with the in-place addend (the buffer keeps accumulating: the time does not depend on its words).
  R1:   `sets` calls of lsr_ntt_ring_fold_batch_device with the weights as constant polynomials, built outside the timed region.  It
        writes [sets][count][width][n] and is compared after a permutation that is not timed.  No addend: the fold cannot add one.

  Shapes, q = 17592169062401 (the FP64 flavour), all vectors in ONE weight group (components = count), term_stride = terms:
  (A) n = 64, width 1024, count 16, terms 256, sets 3 — LaBRADOR's proportions.   (B) n = 4096, width 16, otherwise as (A).
  (C) as (B) with sets 16.                                                        (D) as (B) with terms 16.

env REPS (default 12), WARMUP (2), SHAPES (default "ABCD"), OUT (a JSON file to write, with the provenance stamp), NEW_ONLY=1 (only
the fused calls are timed, back to back: the setting in which two builds of the kernel are compared), LIBVARIANT (an experiment build
of the library, csrc/Makefile VARIANT=...; implies NEW_ONLY), MERGE (a comma separated list of JSON files written by such runs,
embedded under "new_only_runs"), KERNEL_TRACE (a JSON file of per-kernel times read from a rocprofv3 --kernel-trace run of
`NEW_ONLY=1 SHAPES=X`, a process of its own per shape, embedded under "kernel_trace_new_only")."""
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
from ring_project_bench import timed  # noqa: E402

Q = 17592169062401
SHAPES = {"A": (64, 1024, 16, 256, 3), "B": (4096, 16, 16, 256, 3), "C": (4096, 16, 16, 256, 16), "D": (4096, 16, 16, 16, 3)}   # n, width, count, terms, sets
L2SQ_TB_PER_S = 5.8            # what ring_l2sq reads at on this part (profiles/r25_ring_project_bench.json)


def seeded(shape, seed):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    return torch.randint(0, Q, shape, dtype=torch.int64, device="cuda", generator=gen)


def measure(pkg, name, reps, warmup, new_only):
    n, width, count, terms, sets = SHAPES[name]
    length = n * width
    ctx = pkg.NttContext(Q, n, device=0)
    s = torch.cuda.current_stream().cuda_stream
    v = seeded((count * terms, width, n), 28)
    weights = seeded((1, sets, terms), 29)
    addend = seeded((count, sets, width, n), 30)
    out_new, out_plus = torch.empty_like(addend), addend.clone()
    status = torch.empty((2, count), dtype=torch.int32, device="cuda")

    def new():
        ctx.ring_scalar_combine_device(out_new.data_ptr(), status[0].data_ptr(), v.data_ptr(), weights.data_ptr(), 0, count, sets, terms, terms, width, count, s)

    def new_plus():
        ctx.ring_scalar_combine_device(out_plus.data_ptr(), status[1].data_ptr(), v.data_ptr(), weights.data_ptr(), out_plus.data_ptr(), count, sets, terms,
                                       terms, width, count, s)

    routes = [("new", new), ("new+", new_plus)]
    # the in-place form once, from the addend itself, held against the plain form plus the addend
    new()
    new_plus()
    torch.cuda.synchronize()
    total = out_new + addend
    in_place_equal = bool(torch.equal(out_plus, torch.where(total >= Q, total - Q, total)))
    if not new_only:
        consts = torch.zeros((sets, count, terms, n), dtype=torch.int64, device="cuda")
        consts[:, :, :, 0] = weights[0][:, None, :]
        out_r1 = torch.empty((sets, count, width, n), dtype=torch.int64, device="cuda")

        def r1():
            for k in range(sets):
                ctx.ring_fold_device(out_r1[k].data_ptr(), v.data_ptr(), consts[k].data_ptr(), count, terms, terms, width, s)

        routes.append(("R1", r1))
        r1()
        torch.cuda.synchronize()
    per_vector = (terms + sets) * length * 8
    row = {"shape": name, "n": n, "width": width, "count": count, "terms": terms, "sets": sets, "term_stride": terms, "components": count, "q": Q,
           "uses_f64": bool(ctx.uses_f64), "status_all_done": bool((status == 1).all()), "in_place_equals_plain_plus_addend": in_place_equal,
           "bytes_moved_new": count * per_vector, "bytes_moved_new+": count * (per_vector + sets * length * 8)}
    if not new_only:
        row["outputs_equal"] = bool(torch.equal(out_new, out_r1.permute(1, 0, 2, 3)))
    row.update(timed(routes, reps, warmup))
    for which in ("new", "new+"):
        row["%s_TB_per_s" % which] = round(row["bytes_moved_" + which] / row[which]["us_median"] / 1e6, 3)
    row["ring_l2sq_TB_per_s_for_comparison"] = L2SQ_TB_PER_S
    if not new_only:
        row["ratio_R1_over_new"] = round(row["R1"]["us_median"] / row["new"]["us_median"], 2)
        row["new_below_R1_by_more_than_the_spreads"] = bool(row["R1"]["us_median"] - row["new"]["us_median"] > row["R1"]["us_spread"] + row["new"]["us_spread"])
    ctx.close()
    del routes
    torch.cuda.empty_cache()
    return row


def main():
    reps, warmup = int(os.environ.get("REPS", "12")), int(os.environ.get("WARMUP", "2"))
    pkg = entry.load_package()
    variant = os.environ.get("LIBVARIANT")
    if variant:
        pkg._abi.use_library(os.path.join(os.path.dirname(pkg._abi.LIB_PATH), "liblambda_snark_core_%s.so" % variant))
    new_only = bool(variant) or os.environ.get("NEW_ONLY") == "1"
    rows = [measure(pkg, name, reps, warmup, new_only) for name in os.environ.get("SHAPES", "ABCD")]
    out = {"tool": "ring_scalar_combine_bench", "library_variant": variant, "new_only": new_only, "reps": reps, "warmup": warmup, "rows": rows,
           "all_equal": all(r.get("outputs_equal", True) and r["in_place_equals_plain_plus_addend"] for r in rows), "provenance": provenance.provenance()}
    if not new_only:
        out["criterion_met_at_A_and_B"] = all(r["new_below_R1_by_more_than_the_spreads"] for r in rows if r["shape"] in "AB")
    if os.environ.get("MERGE"):
        out["new_only_runs"] = []
        for path in os.environ["MERGE"].split(","):
            with open(path) as f:
                out["new_only_runs"].append(json.load(f))
    if os.environ.get("KERNEL_TRACE"):
        with open(os.environ["KERNEL_TRACE"]) as f:
            out["kernel_trace_new_only"] = json.load(f)
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
