"""The bounded resident-matrix product under an arbitrary modulus (lsr_ring_mod_matvec_bounded_batch_device) against
the calls a caller had before it, on the same seeded device-resident operands, in one process, the routes alternating after a
warm-up.  Prints ONE JSON line.

  (A) cost of the check: the bounded call with bound_x = 0 against lsr_ring_mod_matvec_batch_device at the four shapes of §5q.  Both
      take the same column groups, so the difference is the check (and the gated reduce).
  (B) gain from the bound: q = 2^40 + 15, n = 64, 16 x 258, batch 256, x within 128.  The bounded call at bound_x = 128 (one group)
      against the plain call (37 groups), the gadget call at b = 8 on 43 columns (one group; another operand, the same matrix shape)
      and the by-hand route: two lsr_ring_mod_lift_batch_device, lsr_ntt_ring_matvec_batch_device per prime on matrices resident per
      prime, one lsr_ring_mod_reduce_batch_device, and lsr_ntt_ring_linf_batch_device on the coefficient context for the check.
  (C) a bound that does not change the grouping: n = 4096, q = 2^32, 4 x 16, batch 1024, x within 2^20 (max_terms is 8192 there:
      the 16 columns are one group with or without the bound).
  (A+) one more shape for (A), n = 128.  (Below n = 512 the check runs as a pass of its own, from there on in the tile kernel; an
      experiment build with -DLSR_MOD_MATVEC_CHECK_IN_TILE=1 or =0, measured through LIBRARY, moves it.)

Before timing, the outputs of all routes of a row that compute the same product are asserted equal word for word and every status 1.
env REPS (default 12), WARMUP (2), OUT (a JSON file to write, with the provenance stamp), ONLY (the rows of one n), LIBRARY (an
experiment build of csrc/Makefile VARIANT=... to measure instead of the product library)."""
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
from ring_mod_matvec_bench import timed  # noqa: E402

Q_5_MOD_8 = 4294967197
Q41 = (1 << 40) + 15
# (part, n, q, rows, cols, batch, bound of x's words (0: any word below q), bound_x of the call)
SHAPES = [("A", 64, Q_5_MOD_8, 16, 256, 1024, 0, 0), ("A", 4096, 1 << 32, 4, 16, 1024, 0, 0), ("A", 256, 3329, 4, 4, 16384, 0, 0),
          ("A", 64, Q41, 16, 258, 256, 0, 0), ("A+", 128, Q_5_MOD_8, 8, 64, 2048, 0, 0), ("B", 64, Q41, 16, 258, 256, 128, 128), ("C", 4096, 1 << 32, 4, 16, 1024, 1 << 20, 1 << 20)]


def groups(pkg, q, n, cols, bound):
    capacity = pkg.ring_mod_capacity_bounded(q, n, bound or q // 2)
    return (cols + capacity - 1) // capacity


def measure(pkg, part, n, q, rows, cols, batch, drawn, bound_x, reps, warmup):
    ring = pkg.RingMod(q, n, device=0)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(n + cols + bound_x % 1000)
    s = torch.cuda.current_stream().cuda_stream
    m = torch.randint(0, q, (rows, cols, n), dtype=torch.int64, device="cuda", generator=gen)
    if drawn:
        x = torch.randint(-drawn, drawn + 1, (batch, cols, n), dtype=torch.int64, device="cuda", generator=gen)
        x = torch.where(x < 0, x + q, x)
    else:
        x = torch.randint(0, q, (batch, cols, n), dtype=torch.int64, device="cuda", generator=gen)
    mat = ring.matrix_device(m.data_ptr(), rows, cols, s)
    outs = {name: torch.empty((batch, rows, n), dtype=torch.int64, device="cuda") for name in ("bounded", "plain", "by_hand", "gadget")}
    status = torch.full((batch,), 7, dtype=torch.int32, device="cuda")

    def bounded():
        mat.matvec_bounded_device(outs["bounded"].data_ptr(), status.data_ptr(), x.data_ptr(), batch, bound_x, s)

    def plain():
        mat.matvec_device(outs["plain"].data_ptr(), x.data_ptr(), batch, s)

    routes = [("bounded", bounded), ("plain", plain)]
    closers = [mat]
    if part == "B":
        b = 8
        digits = pkg.ring_gadget_min_digits(q, b)
        xcols = cols // digits
        assert xcols * digits == cols and pkg.ring_mod_capacity_bounded(q, n, 1 << (b - 1)) >= cols
        xg = torch.randint(0, q, (batch, xcols, n), dtype=torch.int64, device="cuda", generator=gen)

        def gadget():
            mat.matvec_gadget_device(outs["gadget"].data_ptr(), xg.data_ptr(), batch, b, digits, s)

        ctxs, coeff = [ring.prime_context(i) for i in range(2)], ring.coeff_context()
        per_prime, tmp = [], torch.empty_like(m)
        for i in range(2):
            ring.lift_device(i, tmp.data_ptr(), m.data_ptr(), m.numel(), s)
            per_prime.append(ctxs[i].ring_matrix_device(tmp.data_ptr(), rows, cols, s))
        closers += per_prime
        lifted = [torch.empty_like(x) for _ in range(2)]
        res = [torch.empty((batch, rows, n), dtype=torch.int64, device="cuda") for _ in range(2)]
        linf = torch.zeros((batch * cols,), dtype=torch.int64, device="cuda")

        def by_hand():
            coeff.ring_linf_device(x.data_ptr(), batch * cols, linf.data_ptr(), s)
            for i in range(2):
                ring.lift_device(i, lifted[i].data_ptr(), x.data_ptr(), x.numel(), s)
                per_prime[i].matvec_device(res[i].data_ptr(), lifted[i].data_ptr(), batch, s)
            ring.reduce_device(outs["by_hand"].data_ptr(), res[0].data_ptr(), res[1].data_ptr(), batch * rows * n, False, s)

        routes += [("gadget", gadget), ("by_hand", by_hand)]
    for _, fn in routes:
        fn()
    torch.cuda.synchronize()
    equal = bool(torch.equal(outs["bounded"], outs["plain"])) and bool((status == 1).all())
    if part == "B":
        equal = equal and bool(torch.equal(outs["bounded"], outs["by_hand"])) and int(linf.max()) <= drawn
    assert equal, (part, n, q, "the routes differ or a status is not 1")
    row = {"part": part, "n": n, "q": q, "rows": rows, "cols": cols, "batch": batch, "x_within": drawn or q // 2, "bound_x": bound_x,
           "groups_bounded": groups(pkg, q, n, cols, bound_x), "groups_plain": groups(pkg, q, n, cols, 0), "outputs_equal": equal,
           "uses_f64": bool(ring.prime_context(0).uses_f64)}
    row.update(timed(routes, reps, warmup))
    row["bounded_minus_plain_us"] = round(row["bounded"]["us_median"] - row["plain"]["us_median"], 1)
    row["sum_of_spreads_us"] = round(row["bounded"]["us_spread"] + row["plain"]["us_spread"], 1)
    for name in ("plain", "gadget", "by_hand"):
        if name in row:
            row["ratio_%s_over_bounded" % name] = round(row[name]["us_median"] / row["bounded"]["us_median"], 2)
    for one in reversed(closers):
        one.close()
    ring.close()
    return row


def main():
    reps, warmup = int(os.environ.get("REPS", "12")), int(os.environ.get("WARMUP", "2"))
    only = os.environ.get("ONLY")
    pkg = entry.load_package()
    if os.environ.get("LIBRARY"):
        pkg._abi.use_library(os.environ["LIBRARY"])
    rows = []
    for shape in SHAPES:
        if only and int(only) != shape[1]:
            continue
        rows.append(measure(pkg, *shape, reps, warmup))
        torch.cuda.empty_cache()
    out = {"tool": "ring_mod_matvec_bounded_bench", "reps": reps, "warmup": warmup, "rows": rows, "all_equal": all(r["outputs_equal"] for r in rows),
           "library": os.environ.get("LIBRARY", ""), "provenance": provenance.provenance()}
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
