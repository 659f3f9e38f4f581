"""The adjoint Pi^T w of the seeded projection (lsr_ntt_ring_project_adjoint_batch_device), whose matrix is generated
inside the kernel that applies it, against the composed route the same library makes possible.  One process, seeded device-resident
operands, the routes alternating after a warm-up, the outputs compared word for word at every shape.  Prints ONE JSON line.

  new: the fused device call.
  R1:  per vector lsr_ntt_ring_project_matrix_batch_device (256 rows, 128 MiB at len 65536), lsr_ntt_ring_fold_batch_device with the
       weights as constant polynomials (256 terms), lsr_ntt_ring_automorphism_batch_device: the composed route end to end.
  R2:  R1 with the matrices of all vectors written OUTSIDE the timed region: the composed route's best case.

  Shapes, q = 17592169062401 (the FP64 flavour), conjugate 1, all vectors in ONE key group (components = count: the witness vectors of
  one proof share their weights, and the constant polynomials of the composed routes stay one set of sets x 256 polynomials):
  (A) n = 64, width 1024, count 16, sets 3 — LaBRADOR's proportions.   (B) n = 4096, width 16, count 16, sets 3.
  (C) as (B) with sets 1 and count 256.                                 (D) as (B) with sets 16.

env REPS (default 12), WARMUP (2), SHAPES (default "ABCD"), OUT (a JSON file to write, with the provenance stamp), NEW_ONLY=1 (only
the fused call is timed, back to back: the setting in which two builds of its kernel are compared), LIBVARIANT (an experiment build
of the library, csrc/Makefile VARIANT=...; implies NEW_ONLY), MERGE (a comma separated list of JSON files written by such runs,
embedded under "new_only_runs")."""
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
from ring_project_bench import random_keys, timed  # noqa: E402

Q, ROWS = 17592169062401, 256
SHAPES = {"A": (64, 1024, 16, 3), "B": (4096, 16, 16, 3), "C": (4096, 16, 256, 1), "D": (4096, 16, 16, 16)}      # n, width, count, sets


def measure(pkg, name, reps, warmup, new_only):
    n, width, count, sets = SHAPES[name]
    length = n * width
    ctx = pkg.NttContext(Q, n, device=0)
    s = torch.cuda.current_stream().cuda_stream
    g = ctx.galois_conjugation
    keys = random_keys(1, 7)
    weights = torch.from_numpy(np.random.default_rng(27).integers(0, Q, size=(1, sets, ROWS), dtype=np.int64)).cuda()
    out_new = torch.empty((count, sets, width, n), dtype=torch.int64, device="cuda")
    status = torch.empty((count,), dtype=torch.int32, device="cuda")

    def new():
        ctx.ring_project_adjoint_device(out_new.data_ptr(), status.data_ptr(), weights.data_ptr(), count, sets, width, 1, keys.data_ptr(), count, 17, 0, s)

    routes = [("new", new)]
    if not new_only:
        # the weights as constant polynomials [sets][256][n], an operand of the composed routes like the weights of the fused one
        consts = torch.zeros((sets, ROWS, n), dtype=torch.int64, device="cuda")
        consts[:, :, 0] = weights[0]
        pi = torch.empty((ROWS, width, n), dtype=torch.int64, device="cuda")
        folded = torch.empty((sets, width, n), dtype=torch.int64, device="cuda")
        out_r1, out_r2 = torch.empty_like(out_new), torch.empty_like(out_new)
        resident = torch.empty((count, ROWS, width, n), dtype=torch.int64, device="cuda")      # count x 128 MiB at len 65536
        for j in range(count):
            ctx.ring_project_matrix_device(resident[j].data_ptr(), 0, ROWS, width, keys.data_ptr(), 17, ROWS * j, s)

        def fold_and_conjugate(matrix, out):
            ctx.ring_fold_device(folded.data_ptr(), matrix.data_ptr(), consts.data_ptr(), sets, ROWS, 0, width, s)
            ctx.ring_automorphism_device(out.data_ptr(), folded.data_ptr(), sets * width, g, s)

        def r1():
            for j in range(count):
                ctx.ring_project_matrix_device(pi.data_ptr(), 0, ROWS, width, keys.data_ptr(), 17, ROWS * j, s)
                fold_and_conjugate(pi, out_r1[j])

        def r2():
            for j in range(count):
                fold_and_conjugate(resident[j], out_r2[j])

        routes += [("R1", r1), ("R2", r2)]
    for _, fn in routes:
        fn()
    torch.cuda.synchronize()
    row = {"shape": name, "n": n, "width": width, "count": count, "sets": sets, "components": count, "conjugate": 1, "q": Q, "uses_f64": bool(ctx.uses_f64),
           "status_all_done": bool((status == 1).all()), "output_bytes": count * sets * length * 8,
           "lane_operations_model": count * length * ROWS * (4 * sets + 2)}
    if not new_only:
        row["outputs_equal"] = bool(torch.equal(out_new, out_r1) and torch.equal(out_new, out_r2))
        row["composed_matrix_bytes_per_vector"] = ROWS * length * 8
    row.update(timed(routes, reps, warmup))
    row["new_G_lane_operations_per_s"] = round(row["lane_operations_model"] / row["new"]["us_median"] / 1e3, 1)
    for other, _ in routes[1:]:
        row["ratio_%s_over_new" % other] = round(row[other]["us_median"] / row["new"]["us_median"], 2)
    if not new_only:
        row["new_below_R2_by_more_than_the_spreads"] = bool(row["R2"]["us_median"] - row["new"]["us_median"] > row["R2"]["us_spread"] + row["new"]["us_spread"])
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
    out = {"tool": "ring_project_adjoint_bench", "library_variant": variant, "new_only": new_only, "reps": reps, "warmup": warmup, "rows": rows,
           "all_equal": all(r.get("outputs_equal", True) for r in rows), "provenance": provenance.provenance()}
    if not new_only:
        out["criterion_met_at_A_and_B"] = all(r["new_below_R2_by_more_than_the_spreads"] for r in rows if r["shape"] in "AB")
    if os.environ.get("MERGE"):
        out["new_only_runs"] = []
        for path in os.environ["MERGE"].split(","):
            with open(path) as f:
                out["new_only_runs"].append(json.load(f))
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
