"""lsr_lwe_combine_rows_device against the only way to combine device-resident rows without it: bring the rows to the host, wrap each in
an LweCommitment, call lwe_linear_combine once per output, upload the results.  n = 4096, rank K, a default and an RNS context, three
shapes, ONE session:
  (a) outputs = 1,    terms = 256,  term_stride = 0
  (b) outputs = 4096, terms = 4,    term_stride = 4      per-proof folding
  (c) outputs = 64,   terms = 1024, term_stride = 0      shared terms
new:    HIP events around the call, REPS repetitions after warm-up, alternating over the shapes; median, spread (max - min), IQR
parent: host clock around download + wrap + loop + upload, ending in a device synchronise; PARENT_REPS repetitions (the loop takes of the
        order of a second per repetition), median and spread, with the share of each stage
The outputs of the two are compared word for word at the timed sizes.  Traffic: the bytes the algorithm needs — term rows read once per
call when they are shared, once per output otherwise, plus the outputs written — over the new call's time, against 8 TB/s.
env: K (2), REPS (20), PARENT_REPS (3), SHAPES (abc), CONTEXTS (default,rns), SKIP_PARENT (0; 1: only the new entry point, for profiler
runs), OUT (a JSON file to write, with the provenance stamp).  Prints one JSON line."""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as entry
import provenance

pkg = entry.load_package()
lib = pkg._abi.lib()
N = 4096
K = int(os.environ.get("K", 2))
REPS, PARENT_REPS = max(10, int(os.environ.get("REPS", 20))), max(1, int(os.environ.get("PARENT_REPS", 3)))
SKIP_PARENT = os.environ.get("SKIP_PARENT", "0") == "1"
ALL_SHAPES = {"a": (1, 256, 0), "b": (4096, 4, 4), "c": (64, 1024, 0)}          # outputs, terms, term_stride
SHAPES = [(name, ALL_SHAPES[name]) for name in os.environ.get("SHAPES", "abc")]
PEAK = 8e12
MSG = 8

rng = np.random.default_rng(15)
s = torch.cuda.current_stream().cuda_stream
out = {"n": N, "k": K, "reps": REPS, "parent_reps": PARENT_REPS, "roofline_bytes_per_s": PEAK}
state = []
for kind in os.environ.get("CONTEXTS", "default,rns").split(","):
    params = pkg.Params(n=N, k=K, sigma=3.19)
    ctx = pkg.LweContext.create_rns(params, key_seed=99, device=0) if kind == "rns" else pkg.LweContext(params, key_seed=99, device=0)
    t, W = ctx.plain_modulus, ctx.commitment_words
    for name, (outputs, terms, stride) in SHAPES:
        count = (outputs - 1) * stride + terms
        msgs = rng.integers(0, t, size=(count, MSG), dtype=np.uint64)
        keys = torch.from_numpy(ctx.commit_keys(msgs, rng.integers(1, 2**63, size=count, dtype=np.uint64)).view(np.int64)).cuda()
        d_msgs = torch.from_numpy(msgs.view(np.int64)).cuda()
        rows = torch.zeros((count, W), dtype=torch.int64, device="cuda")
        ctx.commit_rows_device(d_msgs.data_ptr(), MSG, count, keys.data_ptr(), rows.data_ptr(), s)
        if kind == "rns":            # the reference's range
            coeffs = rng.integers(0, t, size=(outputs, terms), dtype=np.uint64)
        else:                        # inside the budget of a 44-bit context: weight <= 2/3 terms
            coeffs = np.array([1, t - 1, 0], dtype=np.uint64)[(np.arange(outputs * terms) + rng.integers(0, 3)) % 3].reshape(outputs, terms)
        state.append({"kind": kind, "shape": name, "ctx": ctx, "outputs": outputs, "terms": terms, "stride": stride, "rows": rows, "coeffs": coeffs,
                      "d_coeffs": torch.from_numpy(coeffs.view(np.int64)).cuda(), "d_out": torch.zeros((outputs, W), dtype=torch.int64, device="cuda"),
                      "d_status": torch.zeros(outputs, dtype=torch.int32, device="cuda"), "new": [], "parent": [], "stages": []})
torch.cuda.synchronize()


def new_once(st):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    st["ctx"].combine_rows_device(st["rows"].data_ptr(), st["terms"], st["d_coeffs"].data_ptr(), st["outputs"], st["d_out"].data_ptr(), st["d_status"].data_ptr(),
                                  term_stride=st["stride"], stream=s)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def parent_once(st):
    """rows to the host, one LweCommitment per row, one lwe_linear_combine per output, results back to the device -> (ms, stage ms, rows)"""
    ctx, outputs, terms, stride = st["ctx"], st["outputs"], st["terms"], st["stride"]
    W = ctx.commitment_words
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = st["rows"].cpu().numpy().view(np.uint64)
    t1 = time.perf_counter()
    views = [pkg._abi.LweCommitment(host[i].ctypes.data_as(pkg._abi.u64p), W) for i in range(host.shape[0])]
    pointers = [ctypes.pointer(v) for v in views]
    t2 = time.perf_counter()
    result = np.empty((outputs, W), dtype=np.uint64)
    for j in range(outputs):
        arr = (ctypes.POINTER(pkg._abi.LweCommitment) * terms)(*pointers[j * stride:j * stride + terms])
        p = lib.lwe_linear_combine(ctx.handle, arr, st["coeffs"][j].ctypes.data, terms)
        assert p, "the parent refused a combination: " + pkg._abi.last_error()
        ctypes.memmove(result[j].ctypes.data, p.contents.data, W * 8)
        lib.lwe_commitment_free(p)
    t3 = time.perf_counter()
    back = torch.from_numpy(result.view(np.int64)).cuda()
    torch.cuda.synchronize()
    t4 = time.perf_counter()
    return (t4 - t0) * 1e3, [(t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3], back


for _ in range(3):                                   # warm-up: code objects, clocks
    for st in state:
        new_once(st)
for _ in range(REPS):
    for st in state:
        st["new"].append(new_once(st))
if not SKIP_PARENT:
    for rep in range(PARENT_REPS + 1):               # the first repetition warms the host path (pinned staging of the context) and is dropped
        for st in state:
            ms, stages, back = parent_once(st)
            if rep:
                st["parent"].append(ms)
                st["stages"].append(stages)
            else:
                assert int(st["d_status"].sum().item()) == st["outputs"], "every output must be combined"
                assert torch.equal(back, st["d_out"]), "the new entry point and the parent loop differ"
for st in state:
    ctx, outputs, terms, stride = st["ctx"], st["outputs"], st["terms"], st["stride"]
    row_bytes = ctx.commitment_words * 8
    xs = sorted(st["new"])
    e = {"outputs": outputs, "terms": terms, "term_stride": stride, "row_bytes": row_bytes, "new_ms": statistics.median(xs), "new_spread_ms": xs[-1] - xs[0],
         "new_iqr_ms": xs[(3 * len(xs)) // 4] - xs[len(xs) // 4]}
    reads = terms if stride == 0 else outputs * terms
    e["algorithmic_bytes"] = (reads + outputs) * row_bytes + outputs * terms * 8
    e["term_row_reads_counted"] = reads
    e["achieved_bytes_per_s"] = e["algorithmic_bytes"] / (e["new_ms"] * 1e-3)
    e["fraction_of_roofline"] = e["achieved_bytes_per_s"] / PEAK
    e["modular_products"] = outputs * terms * (row_bytes // 8)
    e["products_per_s"] = e["modular_products"] / (e["new_ms"] * 1e-3)
    if st["parent"]:
        ps = sorted(st["parent"])
        e["parent_ms"] = statistics.median(ps)
        e["parent_spread_ms"] = ps[-1] - ps[0]
        e["parent_stage_ms"] = dict(zip(("download", "wrap", "combine_loop", "upload"), [statistics.median(x) for x in zip(*st["stages"])]))
        e["parent_over_new"] = e["parent_ms"] / e["new_ms"]
        e["outputs_equal"] = True
    out.setdefault(st["kind"], {"pipeline": ctx.pipeline})[st["shape"]] = e
out["provenance"] = provenance.provenance()
line = json.dumps(out)
if os.environ.get("OUT"):
    with open(os.environ["OUT"], "w") as f:
        f.write(line + "\n")
print(line)
