"""Two-prime RNS commitments against the two existing routes: device-resident lsr_lwe_commit_rows_device / lsr_lwe_verify_rows_device
at n = 4096 on (a) an RNS context, (b) a default context, (c) an lsr_lwe_wide_modulus context (the other route to the reference's
linear-combine range), timed with HIP events in ONE session: REPS alternating repetitions a, b, c, a, b, c ... after warm-up, median
and run-to-run spread (max - min over the repetitions, and the interquartile range) per configuration.
env: K (rank, 2), J (batch, 16384), MSG (message words, 16), REPS (12), OUT (a JSON file to write, with the provenance stamp).
Prints one JSON line."""
import json
import os
import statistics
import sys

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
K, J = int(os.environ.get("K", 2)), int(os.environ.get("J", 16384))
MSG, REPS = int(os.environ.get("MSG", 16)), max(10, int(os.environ.get("REPS", 12)))

configs = [("rns", pkg.LweContext.create_rns(pkg.Params(n=N, k=K, sigma=3.19), key_seed=99, device=0)),
           ("default", pkg.LweContext(pkg.Params(n=N, k=K, sigma=3.19), key_seed=99, device=0)),
           ("wide", pkg.LweContext(pkg.Params(q=pkg.wide_modulus(N), n=N, k=K, sigma=3.19), key_seed=99, device=0))]
rng = np.random.default_rng(1)
msgs = rng.integers(0, configs[0][1].plain_modulus, size=(J, MSG), dtype=np.uint64)
seeds = rng.integers(1, 2**63, size=J, dtype=np.uint64)
d_msgs = torch.from_numpy(msgs.view(np.int64)).cuda()
s = torch.cuda.current_stream().cuda_stream
state = {}
for name, ctx in configs:
    keys = ctx.commit_keys(msgs, seeds)
    st = {"ctx": ctx, "keys": torch.from_numpy(keys.view(np.int64)).cuda(), "rows": torch.zeros((J, ctx.commitment_words), dtype=torch.int64, device="cuda"),
          "res": torch.zeros(J, dtype=torch.int32, device="cuda"), "commit": [], "verify": []}
    state[name] = st


def once(st, what):
    ctx = st["ctx"]
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    if what == "commit":
        ctx.commit_rows_device(d_msgs.data_ptr(), MSG, J, st["keys"].data_ptr(), st["rows"].data_ptr(), s)
    else:
        ctx.verify_rows_device(st["rows"].data_ptr(), d_msgs.data_ptr(), MSG, J, st["res"].data_ptr(), s)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


for _ in range(3):                                   # warm-up: allocations, code objects, clocks
    for name, _ctx in configs:
        once(state[name], "commit"); once(state[name], "verify")
for _ in range(REPS):
    for what in ("commit", "verify"):
        for name, _ctx in configs:
            state[name][what].append(once(state[name], what))
out = {"n": N, "k": K, "batch": J, "msg_words": MSG, "reps": REPS}
for name, ctx in configs:
    st = state[name]
    assert int(st["res"].sum().item()) == J, "every row must open"
    entry_ = {"pipeline": ctx.pipeline, "row_bytes": ctx.commitment_words * 8}
    for what, unit in (("commit", "commits_per_s"), ("verify", "openings_per_s")):
        xs = sorted(st[what])
        med = statistics.median(xs)
        entry_[what + "_ms"] = med
        entry_[what + "_spread_ms"] = xs[-1] - xs[0]
        entry_[what + "_iqr_ms"] = xs[(3 * len(xs)) // 4] - xs[len(xs) // 4]
        entry_[unit] = J / med * 1e3
    out[name] = entry_


def beats(a, b, what, factor=1.0):
    """a's median below factor * b's by more than the larger of the two spreads"""
    spread = max(out[a][what + "_spread_ms"], factor * out[b][what + "_spread_ms"])
    return out[a][what + "_ms"] + spread < factor * out[b][what + "_ms"]


out["criterion1_rns_beats_wide"] = {"commit": beats("rns", "wide", "commit"), "verify": beats("rns", "wide", "verify")}
out["criterion2_rns_commit_below_twice_default"] = beats("rns", "default", "commit", 2.0)
out["rns_over_default"] = {"commit": out["rns"]["commit_ms"] / out["default"]["commit_ms"], "verify": out["rns"]["verify_ms"] / out["default"]["verify_ms"]}
out["provenance"] = provenance.provenance()
line = json.dumps(out)
if os.environ.get("OUT"):
    with open(os.environ["OUT"], "w") as f:
        f.write(line + "\n")
print(line)
