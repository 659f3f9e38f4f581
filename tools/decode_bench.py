"""Decoding rows against the opening check it shares its pipeline with: device-resident rows at n = 4096 on a default and an RNS context,
timed with HIP events in ONE session.  Per context
  (a) verify    lsr_lwe_verify_rows_device, msg_len = MSG           the existing code: the yardstick
  (b) decode    lsr_lwe_decode_rows_device, slots = MSG, no noise   the same row read once, the same MSG divisions per row
  (c) decode_n  lsr_lwe_decode_rows_device, slots = n, with noise   n divisions and n stored words per row
  (d) decode_q  lsr_lwe_decode_rows_device, slots = MSG, with noise the n divisions of (c) without its stores: splits (c) - (a) into
                arithmetic ((d) - (a)) and written traffic ((c) - (d))
REPS alternating repetitions a, b, c, d, a, b, c, d ... after warm-up; median and run-to-run spread (max - min, and the interquartile
range) per measurement.  Also counts what (c) must move and divide, for the bound named in DESIGN.md section 6b.
env: K (rank, 2), J (batch, 16384), MSG (16), REPS (12), OUT (a JSON file to write, with the provenance stamp).  Prints one JSON line."""
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
N = 4096
K, J = int(os.environ.get("K", 2)), int(os.environ.get("J", 16384))
MSG, REPS = int(os.environ.get("MSG", 16)), max(10, int(os.environ.get("REPS", 12)))

configs = [("default", pkg.LweContext(pkg.Params(n=N, k=K, sigma=3.19), key_seed=99, device=0)),
           ("rns", pkg.LweContext.create_rns(pkg.Params(n=N, k=K, sigma=3.19), key_seed=99, device=0))]
rng = np.random.default_rng(1)
msgs = rng.integers(0, configs[0][1].plain_modulus, size=(J, MSG), dtype=np.uint64)
seeds = rng.integers(1, 2**63, size=J, dtype=np.uint64)
d_msgs = torch.from_numpy(msgs.view(np.int64)).cuda()
s = torch.cuda.current_stream().cuda_stream
WHAT = ("verify", "decode", "decode_n", "decode_q")
state = {}
for name, ctx in configs:
    keys = torch.from_numpy(ctx.commit_keys(msgs, seeds).view(np.int64)).cuda()
    rows = torch.zeros((J, ctx.commitment_words), dtype=torch.int64, device="cuda")
    ctx.commit_rows_device(d_msgs.data_ptr(), MSG, J, keys.data_ptr(), rows.data_ptr(), s)
    state[name] = {"ctx": ctx, "rows": rows, "res": torch.zeros(J, dtype=torch.int32, device="cuda"), "status": torch.zeros(J, dtype=torch.int32, device="cuda"),
                   "bits": torch.zeros(J, dtype=torch.int32, device="cuda"), "few": torch.zeros((J, MSG), dtype=torch.int64, device="cuda"),
                   "all": torch.zeros((J, N), dtype=torch.int64, device="cuda"), **{w: [] for w in WHAT}}
torch.cuda.synchronize()


def once(st, what):
    ctx = st["ctx"]
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    if what == "verify":
        ctx.verify_rows_device(st["rows"].data_ptr(), d_msgs.data_ptr(), MSG, J, st["res"].data_ptr(), s)
    elif what == "decode":
        ctx.decode_rows_device(st["rows"].data_ptr(), J, MSG, st["few"].data_ptr(), st["status"].data_ptr(), None, s)
    elif what == "decode_n":
        ctx.decode_rows_device(st["rows"].data_ptr(), J, N, st["all"].data_ptr(), st["status"].data_ptr(), st["bits"].data_ptr(), s)
    else:
        ctx.decode_rows_device(st["rows"].data_ptr(), J, MSG, st["few"].data_ptr(), st["status"].data_ptr(), st["bits"].data_ptr(), s)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


for _ in range(3):                                   # warm-up: allocations, code objects, clocks
    for name, _ctx in configs:
        for what in WHAT:
            once(state[name], what)
for _ in range(REPS):
    for name, _ctx in configs:
        for what in WHAT:
            state[name][what].append(once(state[name], what))
out = {"n": N, "k": K, "batch": J, "msg_words": MSG, "reps": REPS}
for name, ctx in configs:
    st = state[name]
    assert int(st["res"].sum().item()) == J and int(st["status"].sum().item()) == J, "every row must open and decode"
    assert torch.equal(st["few"], d_msgs) and torch.equal(st["all"][:, :MSG], d_msgs) and not bool(st["all"][:, MSG:].any()), "decoded messages differ"
    entry_ = {"pipeline": ctx.pipeline, "row_bytes": ctx.commitment_words * 8, "noise_bits_min_max": [int(st["bits"].min().item()), int(st["bits"].max().item())],
              "capacity_bits": ctx.noise_capacity_bits}
    for what in WHAT:
        xs = sorted(st[what])
        entry_[what + "_ms"] = statistics.median(xs)
        entry_[what + "_spread_ms"] = xs[-1] - xs[0]
        entry_[what + "_iqr_ms"] = xs[(3 * len(xs)) // 4] - xs[len(xs) // 4]
    entry_["decode_over_verify"] = entry_["decode_ms"] / entry_["verify_ms"]
    entry_["decode_n_over_verify"] = entry_["decode_n_ms"] / entry_["verify_ms"]
    entry_["decode_q_over_verify"] = entry_["decode_q_ms"] / entry_["verify_ms"]
    entry_["decode_within_combined_spreads_of_verify"] = abs(entry_["decode_ms"] - entry_["verify_ms"]) <= entry_["decode_spread_ms"] + entry_["verify_spread_ms"]
    # what (c) needs: the row read once, n slots written; and the achieved rate over those bytes
    moved = J * (ctx.commitment_words * 8 + N * 8)
    entry_["decode_n_bytes"] = moved
    entry_["decode_n_gbytes_per_s"] = moved / entry_["decode_n_ms"] / 1e6
    entry_["verify_gbytes_per_s"] = J * ctx.commitment_words * 8 / entry_["verify_ms"] / 1e6
    entry_["decode_n_divisions"] = J * N
    out[name] = entry_
out["provenance"] = provenance.provenance()
line = json.dumps(out)
if os.environ.get("OUT"):
    with open(os.environ["OUT"], "w") as f:
        f.write(line + "\n")
print(line)
