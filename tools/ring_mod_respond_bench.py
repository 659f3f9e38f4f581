"""Masked responses z = y + sum c s with a verified abort under an arbitrary modulus: the fused lsr_ring_mod_respond_batch_device
against the route composed from the public pieces of the same handle, on the same seeded device-resident operands, in one process, the
routes alternating after a warm-up.  Prints ONE JSON line.

  new:        the fused call with the bounds of the row.
  route:      what a caller composes without it: RingMod.fold_device, a torch add and a remainder mod q, ring_linf_device on the
              handle's coefficient context, and a masked zero over the outputs whose largest word exceeds bound_z.  Four passes over
              out behind the fold; the rejected z lies complete in memory until the last of them.  (The route does not hold y against
              q and bound_y; the fused call does.)
  plain:      the fused call with y == NULL and bound_z == 0, which equals the fold word for word, against
  fold:       RingMod.fold_device: the price of the finish pass and of the new reduce.

Shapes: (a), (l) and (g258) of tools/ring_mod_fold_bench.py — n = 4096, q = 2^32, 1024 outputs x 4 disjoint terms x width 16; n = 64,
q = 4294967197, 16 outputs x 32 disjoint terms x width 1024; n = 64, q = 2^40 + 15, 64 outputs x 258 disjoint terms x width 64 with the
challenges within 2 — and (d) a Dilithium-like round: n = 256, q = 8380417, width 5, one shared secret within 2, 16384 instances with
ball challenges of weight 60, masks within 2^19, bound_z = 2^19 - 120.  On the first three the mask is target - f for a target within
bound_z, every fourth output with one word over it; on (d) the masks are uniform and the protocol rejects what it rejects.
Outputs must be equal word for word and statuses one to one before anything is timed.
Not measured: the host forms, the integer flavour, n < 64.
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
from ring_mod_fold_bench import Q41, Q_5_MOD_8, timed  # noqa: E402

# (label, n, q, outputs, terms, term_stride, width, bound_y, bound_v, bound_p, bound_z)
SHAPES = [("a", 4096, 1 << 32, 1024, 4, 4, 16, 0, 0, 0, 1 << 24), ("l", 64, Q_5_MOD_8, 16, 32, 32, 1024, 0, 0, 0, 1 << 24),
          ("g258", 64, Q41, 64, 258, 258, 64, 0, 0, 2, 1 << 24), ("d", 256, 8380417, 16384, 1, 0, 5, 1 << 19, 2, 1, (1 << 19) - 120)]
BALL_WEIGHT = 60


def short(gen, q, shape, bound):
    return torch.randint(-bound, bound + 1, shape, dtype=torch.int64, device="cuda", generator=gen) % q


def measure(pkg, label, n, q, outputs, terms, stride, width, bound_y, bound_v, bound_p, bound_z, reps, warmup):
    ring = pkg.RingMod(q, n, device=0)
    coeff = ring.coeff_context()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(n + terms + width)
    s = torch.cuda.current_stream().cuda_stream
    vectors = (outputs - 1) * stride + terms
    v = short(gen, q, (vectors, width, n), bound_v) if bound_v else torch.randint(0, q, (vectors, width, n), dtype=torch.int64, device="cuda", generator=gen)
    if label == "d":
        p = torch.empty((outputs, terms, n), dtype=torch.int64, device="cuda")
        key = torch.from_numpy(pkg.ring_sample_key(n).view(np.int64)).cuda()
        coeff.ring_sample_device(p.data_ptr(), outputs, pkg.RING_SAMPLE_BALL, BALL_WEIGHT, key.data_ptr(), outputs, stream=s)
    elif bound_p:
        p = short(gen, q, (outputs, terms, n), bound_p)
    else:
        p = torch.randint(0, q, (outputs, terms, n), dtype=torch.int64, device="cuda", generator=gen)
    outs = {name: torch.empty((outputs, width, n), dtype=torch.int64, device="cuda") for name in ("new", "route", "plain", "fold")}
    status = {name: torch.zeros(outputs, dtype=torch.int32, device="cuda") for name in outs}
    linf = torch.empty((outputs, width), dtype=torch.int64, device="cuda")

    def fold():
        ring.fold_device(outs["fold"].data_ptr(), status["fold"].data_ptr(), v.data_ptr(), p.data_ptr(), outputs, terms, stride, width, bound_v, bound_p, s)

    fold()
    torch.cuda.synchronize()
    if label == "d":
        y = short(gen, q, (outputs, width, n), bound_y)
    else:   # target - f, every fourth output with one word over the bound
        target = short(gen, q, (outputs, width, n), bound_z)
        target[::4, width - 1, n - 1] = q - bound_z - 1
        y = (target - outs["fold"]) % q

    def new():
        ring.respond_device(outs["new"].data_ptr(), status["new"].data_ptr(), y.data_ptr(), v.data_ptr(), p.data_ptr(), outputs, terms, stride, width,
                            bound_y, bound_v, bound_p, bound_z, s)

    def route():
        z = outs["route"]
        ring.fold_device(z.data_ptr(), status["fold"].data_ptr(), v.data_ptr(), p.data_ptr(), outputs, terms, stride, width, bound_v, bound_p, s)
        torch.add(z, y, out=z)
        torch.remainder(z, q, out=z)
        coeff.ring_linf_device(z.data_ptr(), outputs * width, linf.data_ptr(), s)
        rejected = (linf > bound_z).any(dim=1)
        z.masked_fill_(rejected[:, None, None], 0)
        status["route"].copy_(torch.where(rejected, 2, 1))

    def plain():
        ring.respond_device(outs["plain"].data_ptr(), status["plain"].data_ptr(), 0, v.data_ptr(), p.data_ptr(), outputs, terms, stride, width, 0, bound_v,
                            bound_p, 0, s)

    routes = (("new", new), ("route", route), ("plain", plain), ("fold", fold))
    for _, fn in routes:
        fn()
    torch.cuda.synchronize()
    accepted = int((status["new"] == 1).sum())
    equal = bool(torch.equal(outs["new"], outs["route"])) and bool(torch.equal(status["new"], status["route"])) and \
        bool(torch.equal(outs["plain"], outs["fold"])) and bool(torch.equal(status["plain"], status["fold"])) and bool((status["fold"] == 1).all())
    row = {"shape": label, "n": n, "q": q, "outputs": outputs, "terms": terms, "term_stride": stride, "width": width, "bound_y": bound_y,
           "bound_v": bound_v, "bound_p": bound_p, "bound_z": bound_z, "accepted": accepted, "rejected": int((status["new"] == 2).sum()),
           "outputs_equal": equal}
    if not equal or accepted in (0, outputs):
        raise SystemExit("ring_mod_respond_bench: the routes disagree, or one verdict is missing, on shape %s: %s" % (label, json.dumps(row)))
    row.update(timed(routes, reps, warmup))
    row["ratio_route_over_new"] = round(row["route"]["us_median"] / row["new"]["us_median"], 2)
    row["ratio_plain_over_fold"] = round(row["plain"]["us_median"] / row["fold"]["us_median"], 2)
    ring.close()
    return row


def main():
    reps, warmup = int(os.environ.get("REPS", "12")), int(os.environ.get("WARMUP", "2"))
    pkg = entry.load_package()
    rows = []
    for shape in SHAPES:
        rows.append(measure(pkg, *shape, reps, warmup))
        torch.cuda.empty_cache()
    out = {"tool": "ring_mod_respond_bench", "reps": reps, "warmup": warmup, "rows": rows, "all_equal": all(r["outputs_equal"] for r in rows),
           "not_measured": ["host forms", "integer flavour", "n < 64"], "provenance": provenance.provenance()}
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
