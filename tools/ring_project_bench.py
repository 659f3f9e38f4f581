"""The seeded Johnson-Lindenstrauss projection p = Pi s (lsr_ntt_ring_project_batch_device), whose matrix is generated inside the
kernel that applies it, against the composed route the same library makes possible — lsr_ntt_ring_project_matrix_batch_device into a
buffer, the words centred to FP64, a torch (rocBLAS) FP64 product — and the exact l2 norm (lsr_ntt_ring_l2sq_batch_device) beside
lsr_ntt_ring_linf_batch_device on the same buffer.  One process, seeded device-resident operands, the routes alternating after a
warm-up.  Prints ONE JSON line.

  n = 4096, width 16 (len 65536), bound 2^20, q = 17592169062401: len * bound = 2^36 < 2^53, so the FP64 route is exact and the two
  routes are compared word for word.
  (a) 256 vectors, each under its own key (components = 1): the protocol's case.  composed: per vector, the 256 x 65536 matrix
      written (128 MiB), centred to FP64 and multiplied with the centred vector.
  (b) 1024 vectors under ONE key (the key repeated, components = 1): the fused call regenerates the matrix for every vector.
      resident: the centred FP64 matrix built once OUTSIDE the timed region, the timed part centres the vectors and runs one FP64
      GEMM; composed: the same with the matrix generated and centred inside the timed region.
  l2: n = 4096 x 16384 polynomials as 16384 vectors of width 1; rates in TB/s of the 8 bytes a word both calls read.

env REPS (default 12), WARMUP (2), OUT (a JSON file to write, with the provenance stamp), FUSED_ONLY=1 (only the fused projection
is timed, back to back: the setting in which two builds of its kernel are compared — beside the FP64 routes the same kernel runs
3 to 15 % slower), LIBVARIANT (an experiment build of the library, csrc/Makefile VARIANT=...; implies FUSED_ONLY), MERGE (a comma
separated list of JSON files written by such runs, embedded under "fused_only_runs")."""
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

Q, N, WIDTH, BOUND, ROWS = 17592169062401, 4096, 16, 1 << 20, 256
LEN = N * WIDTH


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


def centre(words):
    """canonical int64 words in [0, q) -> centred FP64"""
    return torch.where(words > Q // 2, words - Q, words).to(torch.float64)


def short_vectors(count, seed):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    v = torch.randint(-BOUND, BOUND + 1, (count, LEN), dtype=torch.int64, device="cuda", generator=gen)
    return torch.where(v < 0, v + Q, v)


def random_keys(count, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 2**64, size=(count, 4), dtype=np.uint64).view(np.int64)).cuda()


def measure_project(ctx, count, shared, reps, warmup, fused_only):
    s = torch.cuda.current_stream().cuda_stream
    x = short_vectors(count, 100 + count)
    keys = random_keys(1, 7).repeat(count, 1).contiguous() if shared else random_keys(count, 7)
    out_new = torch.empty((count, ROWS), dtype=torch.int64, device="cuda")
    status = torch.empty((count,), dtype=torch.int32, device="cuda")
    out_composed = torch.empty((count, ROWS), dtype=torch.int64, device="cuda")
    out_resident = torch.empty((count, ROWS), dtype=torch.int64, device="cuda")
    pi = torch.empty((ROWS, LEN), dtype=torch.int64, device="cuda")

    def new():
        ctx.ring_project_device(out_new.data_ptr(), status.data_ptr(), x.data_ptr(), count, WIDTH, BOUND, keys.data_ptr(), 1, 17, 0, s)

    def composed_own():      # every vector its own matrix
        sf = centre(x)
        for j in range(count):
            ctx.ring_project_matrix_device(pi.data_ptr(), 0, ROWS, WIDTH, keys[j].data_ptr(), 17, 0, s)
            out_composed[j] = torch.mv(centre(pi), sf[j]).to(torch.int64)

    def composed_shared():   # one matrix, generated inside the timed region
        ctx.ring_project_matrix_device(pi.data_ptr(), 0, ROWS, WIDTH, keys.data_ptr(), 17, 0, s)
        out_composed.copy_(torch.matmul(centre(x), centre(pi).t()).to(torch.int64))

    routes = [("new", new)]
    if not fused_only:
        routes.append(("composed", composed_shared if shared else composed_own))
        if shared:
            ctx.ring_project_matrix_device(pi.data_ptr(), 0, ROWS, WIDTH, keys.data_ptr(), 17, 0, s)
            pi_resident = centre(pi).t().contiguous()

            def resident():
                out_resident.copy_(torch.matmul(centre(x), pi_resident).to(torch.int64))
            routes.append(("resident", resident))
    for _, fn in routes:
        fn()
    torch.cuda.synchronize()
    row = {"op": "project", "n": N, "width": WIDTH, "bound": BOUND, "q": Q, "count": count, "shared_matrix": shared,
           "status_all_done": bool((status == 1).all()), "entries": count * ROWS * LEN}
    if not fused_only:
        row["outputs_equal"] = bool(torch.equal(out_new, out_composed) and (not shared or torch.equal(out_new, out_resident)))
    row.update(timed(routes, reps, warmup))
    row["new_G_entries_per_s"] = round(row["entries"] / row["new"]["us_median"] / 1e3, 1)
    for name, _ in routes[1:]:
        row["ratio_%s_over_new" % name] = round(row[name]["us_median"] / row["new"]["us_median"], 2)
    return row


def measure_l2(ctx, polys, reps, warmup):
    s = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda")
    gen.manual_seed(polys)
    x = torch.randint(0, Q, (polys, N), dtype=torch.int64, device="cuda", generator=gen)
    l2 = torch.empty((polys, 2), dtype=torch.int64, device="cuda")
    linf = torch.empty((polys,), dtype=torch.int64, device="cuda")

    def new():
        ctx.ring_l2sq_device(x.data_ptr(), polys, 1, l2.data_ptr(), s)

    def route():
        ctx.ring_linf_device(x.data_ptr(), polys, linf.data_ptr(), s)

    routes = (("l2sq", new), ("linf", route))
    row = {"op": "l2sq", "n": N, "q": Q, "polys": polys}
    row.update(timed(routes, reps, warmup))
    for name, _ in routes:
        row[name + "_TBps"] = round(8.0 * polys * N / row[name]["us_median"] / 1e6, 2)
    row["l2sq_within_linf_spread"] = bool(row["l2sq"]["us_median"] <= row["linf"]["us_median"] + row["linf"]["us_spread"])
    # one vector checked against Python integers
    first = x[0].cpu().tolist()
    want = sum((v if v <= Q // 2 else v - Q) ** 2 for v in first)
    got = l2[0].cpu().numpy().view(np.uint64).tolist()
    row["first_vector_exact"] = bool(int(got[0]) | (int(got[1]) << 64) == want)
    return row


def main():
    reps, warmup = int(os.environ.get("REPS", "12")), int(os.environ.get("WARMUP", "2"))
    pkg = entry.load_package()
    variant = os.environ.get("LIBVARIANT")
    if variant:
        pkg._abi.use_library(os.path.join(os.path.dirname(pkg._abi.LIB_PATH), "liblambda_snark_core_%s.so" % variant))
    fused_only = bool(variant) or os.environ.get("FUSED_ONLY") == "1"
    ctx = pkg.NttContext(Q, N, device=0)
    rows = []
    for count, shared in [(256, False), (1024, True)]:
        rows.append(measure_project(ctx, count, shared, reps, warmup, fused_only))
        torch.cuda.empty_cache()
    if not fused_only:
        rows.append(measure_l2(ctx, 16384, reps, warmup))
    ctx.close()
    out = {"tool": "ring_project_bench", "library_variant": variant, "fused_only": fused_only, "reps": reps, "warmup": warmup, "rows": rows,
           "all_equal": all(r.get("outputs_equal", True) for r in rows), "provenance": provenance.provenance()}
    if os.environ.get("MERGE"):
        out["fused_only_runs"] = []
        for path in os.environ["MERGE"].split(","):
            with open(path) as f:
                out["fused_only_runs"].append(json.load(f))
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
