"""Resident-matrix products under an arbitrary modulus: the fused lsr_ring_mod_matvec_batch_device and
lsr_ring_mod_matvec_gadget_batch_device against the route composed from the public pieces of the same handle, on the same seeded
device-resident operands, in one process, the routes alternating after a warm-up.  Prints ONE JSON line.

  new:        the fused call on a resident LsrRingModMatrix.
  route:      the composed route.  Its matrices stay resident and untimed: one LsrRingMatrix per prime context and column group
              (groups of max_terms columns, as batch.h tells a composing caller), made from the lifted columns.  Per call: two
              lsr_ring_mod_lift_batch_device of x, then per group two lsr_ntt_ring_matvec_batch_device and one
              lsr_ring_mod_reduce_batch_device (accumulating from the second group on).  The route reads x in group-major layout
              ([group][batch][columns of the group][n]); for the plain shapes that copy of x is prepared outside the timed region.
  decompose:  (gadget shape only) a ring_decompose under q does not exist: torch integer operations take x to its digits mod q,
              written in the route's group-major layout.  Timed on its own; the gadget route is decompose + route.
  floor:      (information) ONE ordinary lsr_ntt_ring_matvec_batch_device on the first prime's context with all columns: a product
              at an NTT prime.  Two primes should cost about twice it.

Shapes: n = 64, q = 4294967197 (the largest prime = 5 (mod 8) below 2^32), rows 16, cols 256, batch 1024; n = 4096, q = 2^32, rows 4,
cols 16, batch 1024; n = 256, q = 3329, rows 4, cols 4, batch 16384; n = 64, q = 2^40 + 15, rows 16, cols 258, batch 256, once plain
(37 groups of max_terms = 7) and once as the gadget product at b = 8, xcols 43 (one group; the route runs its 37 on the digits).
The outputs of the routes must be equal word for word.
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
# (n, q, rows, cols, batch, base_log2 or None)
SHAPES = [(64, Q_5_MOD_8, 16, 256, 1024, None), (4096, 1 << 32, 4, 16, 1024, None), (256, 3329, 4, 4, 16384, None), (64, Q41, 16, 258, 256, None),
          (64, Q41, 16, 258, 256, 8)]


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


def torch_digits(x, q, b, digits):
    """x [batch][xcols][n] int64 words mod q -> [batch][xcols digits][n] digit residues mod q (batch.h's G^-1 against q)"""
    base = 1 << b
    off = (base // 2) * ((base**digits - 1) // (base - 1))
    u = torch.where(x > q // 2, x - q, x) + off
    z = torch.stack([((u >> (b * d)) & (base - 1)) - base // 2 for d in range(digits)], dim=2)      # [batch][xcols][digits][n]
    z = torch.where(z < 0, z + q, z)
    return z.reshape(x.shape[0], x.shape[1] * digits, x.shape[2])


def measure(pkg, n, q, rows, cols, batch, b, reps, warmup):
    ring = pkg.RingMod(q, n, device=0)
    ctxs = [ring.prime_context(i) for i in range(2)]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(n + cols + (b or 0))
    s = torch.cuda.current_stream().cuda_stream
    digits = pkg.ring_gadget_min_digits(q, b) if b else 1
    xcols = cols // digits
    assert xcols * digits == cols
    m = torch.randint(0, q, (rows, cols, n), dtype=torch.int64, device="cuda", generator=gen)
    x = torch.randint(0, q, (batch, xcols, n), dtype=torch.int64, device="cuda", generator=gen)
    mat = ring.matrix_device(m.data_ptr(), rows, cols, s)
    # the route's resident matrices: per column group and prime, from the lifted columns
    group = min(cols, ring.max_terms)
    bounds = [(g0, min(g0 + group, cols)) for g0 in range(0, cols, group)]
    mats, tmp = [], torch.empty_like(m)
    for g0, g1 in bounds:
        m_g = m[:, g0:g1].contiguous()
        per_prime = []
        for i in range(2):
            ring.lift_device(i, tmp.data_ptr(), m_g.data_ptr(), m_g.numel(), s)
            per_prime.append(ctxs[i].ring_matrix_device(tmp.data_ptr(), rows, g1 - g0, s))
        mats.append(per_prime)
    lifted_m = torch.empty_like(m)
    ring.lift_device(0, lifted_m.data_ptr(), m.data_ptr(), m.numel(), s)
    floor_mat = ctxs[0].ring_matrix_device(lifted_m.data_ptr(), rows, cols, s)
    torch.cuda.synchronize()

    grouped = torch.empty(batch * cols * n, dtype=torch.int64, device="cuda")                  # [group][batch][columns of the group][n]
    offsets = [batch * g0 * n for g0, _ in bounds]

    def regroup(z):
        for (g0, g1), at in zip(bounds, offsets):
            grouped[at:at + batch * (g1 - g0) * n].view(batch, g1 - g0, n).copy_(z[:, g0:g1])

    if not b:
        regroup(x)
    lifted = [torch.empty_like(grouped) for _ in range(2)]
    res = [torch.empty((batch, rows, n), dtype=torch.int64, device="cuda") for _ in range(2)]
    outs = {name: torch.empty((batch, rows, n), dtype=torch.int64, device="cuda") for name in ("new", "route", "floor")}
    x_full = torch_digits(x, q, b, digits) if b else x                                        # the floor's operand: all columns

    def new():
        if b:
            mat.matvec_gadget_device(outs["new"].data_ptr(), x.data_ptr(), batch, b, digits, s)
        else:
            mat.matvec_device(outs["new"].data_ptr(), x.data_ptr(), batch, s)

    def decompose():
        regroup(torch_digits(x, q, b, digits))

    def route():
        for i in range(2):
            ring.lift_device(i, lifted[i].data_ptr(), grouped.data_ptr(), grouped.numel(), s)
        for g, at in enumerate(offsets):
            for i in range(2):
                mats[g][i].matvec_device(res[i].data_ptr(), lifted[i].data_ptr() + 8 * at, batch, s)
            ring.reduce_device(outs["route"].data_ptr(), res[0].data_ptr(), res[1].data_ptr(), batch * rows * n, g > 0, s)

    def floor():
        floor_mat.matvec_device(outs["floor"].data_ptr(), x_full.data_ptr(), batch, s)

    routes = (("new", new),) + ((("decompose", decompose),) if b else ()) + (("route", route), ("floor", floor))
    for _, fn in routes:
        fn()
    torch.cuda.synchronize()
    row = {"op": "ring_mod_matvec_gadget" if b else "ring_mod_matvec", "n": n, "q": q, "rows": rows, "cols": cols, "batch": batch,
           "max_terms": ring.max_terms, "route_groups": len(bounds), "outputs_equal": bool(torch.equal(outs["new"], outs["route"]))}
    if b:
        row.update({"base_log2": b, "digits": digits, "xcols": xcols, "capacity_bounded": pkg.ring_mod_capacity_bounded(q, n, 1 << (b - 1))})
    row.update(timed(routes, reps, warmup))
    route_us = row["route"]["us_median"] + (row["decompose"]["us_median"] if b else 0.0)
    row["route_total_us_median"] = round(route_us, 1)
    row["ratio_route_over_new"] = round(route_us / row["new"]["us_median"], 2)
    row["ratio_new_over_floor"] = round(row["new"]["us_median"] / row["floor"]["us_median"], 2)
    for per_prime in mats:
        for one in per_prime:
            one.close()
    floor_mat.close()
    mat.close()
    ring.close()
    return row


def main():
    reps, warmup = int(os.environ.get("REPS", "12")), int(os.environ.get("WARMUP", "2"))
    pkg = entry.load_package()
    rows = []
    for n, q, n_rows, cols, batch, b in SHAPES:
        rows.append(measure(pkg, n, q, n_rows, cols, batch, b, reps, warmup))
        torch.cuda.empty_cache()
    out = {"tool": "ring_mod_matvec_bench", "reps": reps, "warmup": warmup, "rows": rows, "all_equal": all(r["outputs_equal"] for r in rows),
           "provenance": provenance.provenance()}
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
