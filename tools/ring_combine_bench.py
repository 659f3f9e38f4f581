"""lsr_lwe_ring_combine_rows_device against the only route to the same rows without it on a default context: a torch gather of the row
components into [outputs (k + 1)][terms][n], a torch lift of the polynomials to residues mod q (repeated per component),
lsr_ntt_ring_dot_batch_device through lsr_lwe_ntt_context, and a torch scatter of the results into rows behind a header.
n = 4096, rank K, device-resident, ONE session, two shapes:
  (b) outputs = 4096, terms = 4,   term_stride = 4      disjoint groups
  (c) outputs = 64,   terms = 256, term_stride = 0      shared terms
HIP events around each route, REPS (12) alternating repetitions after warm-up; median and spread (max - min).  The outputs of the two
routes are compared word for word.  Criterion: new median + new spread < composed median on both shapes.  An RNS context has no
composed route (lsr_lwe_ntt_context refuses it): its time is reported beside twice the default context's time.
env: K (2), REPS (12), OUT (a JSON file to write, with the provenance stamp).  Prints one JSON line."""
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
K = int(os.environ.get("K", 2))
REPS = max(12, int(os.environ.get("REPS", 12)))
SHAPES = [("b", (4096, 4, 4)), ("c", (64, 256, 0))]          # outputs, terms, term_stride
MSG = 8

rng = np.random.default_rng(17)
s = torch.cuda.current_stream().cuda_stream
out = {"n": N, "k": K, "reps": REPS}
state = []
for kind in ("default", "rns"):
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
        # two taps of +-1 per polynomial: inside the budget of a 44-bit context at both shapes (weight 2 terms <= 512)
        polys = torch.zeros((outputs, terms, N), dtype=torch.int64, device="cuda")
        taps = torch.from_numpy(rng.integers(0, N, size=(outputs, terms, 2))).cuda()
        polys.scatter_(2, taps, torch.tensor([1, t - 1], dtype=torch.int64, device="cuda").expand(outputs, terms, 2))
        state.append({"kind": kind, "shape": name, "ctx": ctx, "outputs": outputs, "terms": terms, "stride": stride, "rows": rows, "polys": polys,
                      "d_out": torch.zeros((outputs, W), dtype=torch.int64, device="cuda"), "d_status": torch.zeros(outputs, dtype=torch.int32, device="cuda"),
                      "composed_out": torch.zeros((outputs, W), dtype=torch.int64, device="cuda") if kind == "default" else None, "new": [], "composed": []})
torch.cuda.synchronize()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def new_route(st):
    st["ctx"].ring_combine_rows_device(st["rows"].data_ptr(), st["terms"], st["polys"].data_ptr(), st["outputs"], st["d_out"].data_ptr(),
                                       st["d_status"].data_ptr(), term_stride=st["stride"], stream=s)


def composed_route(st):
    ctx, outputs, terms = st["ctx"], st["outputs"], st["terms"]
    q, t, head, kp1 = ctx.commit_modulus, ctx.plain_modulus, 5, K + 1
    body = st["rows"][:, head:].view(-1, kp1, N)
    if st["stride"] == 0:
        a = body.permute(1, 0, 2).unsqueeze(0).expand(outputs, kp1, terms, N).contiguous()
    else:
        a = body.view(outputs, terms, kp1, N).permute(0, 2, 1, 3).contiguous()
    p = st["polys"]
    lifted = torch.where(p > t // 2, p - t + q, p)
    b = lifted.unsqueeze(1).expand(outputs, kp1, terms, N).contiguous()
    c = torch.empty((outputs, kp1, N), dtype=torch.int64, device="cuda")
    rc = lib.lsr_ntt_ring_dot_batch_device(lib.lsr_lwe_ntt_context(ctx.handle), c.data_ptr(), a.data_ptr(), b.data_ptr(), outputs * kp1, terms, outputs * kp1, s)
    assert rc == 0, pkg._abi.last_error()
    st["composed_out"][:, :head] = st["rows"][0, :head]
    st["composed_out"][:, head:] = c.view(outputs, kp1 * N)


for st in state:                     # warm-up: workspaces, code objects
    for _ in range(2):
        new_route(st)
        if st["composed_out"] is not None:
            composed_route(st)
torch.cuda.synchronize()
for _ in range(REPS):                # alternating over contexts, shapes and routes
    for st in state:
        st["new"].append(timed(lambda: new_route(st)))
        if st["composed_out"] is not None:
            st["composed"].append(timed(lambda: composed_route(st)))

for st in state:
    assert st["d_status"].cpu().tolist() == [1] * st["outputs"], (st["kind"], st["shape"])
    xs = sorted(st["new"])
    e = {"outputs": st["outputs"], "terms": st["terms"], "term_stride": st["stride"], "new_ms": statistics.median(xs), "new_spread_ms": xs[-1] - xs[0]}
    if st["composed_out"] is not None:
        assert torch.equal(st["d_out"], st["composed_out"]), (st["kind"], st["shape"])
        cs = sorted(st["composed"])
        e.update({"composed_ms": statistics.median(cs), "composed_spread_ms": cs[-1] - cs[0], "outputs_equal": True})
        e["composed_over_new"] = e["composed_ms"] / e["new_ms"]
        e["criterion_new_median_plus_spread_below_composed_median"] = e["new_ms"] + e["new_spread_ms"] < e["composed_ms"]
    else:
        default = out["default"][st["shape"]]
        e["twice_default_new_ms"] = 2 * default["new_ms"]
        e["rns_over_default"] = e["new_ms"] / default["new_ms"]
    out.setdefault(st["kind"], {"pipeline": st["ctx"].pipeline})[st["shape"]] = e
out["provenance"] = provenance.provenance()
line = json.dumps(out)
if os.environ.get("OUT"):
    with open(os.environ["OUT"], "w") as f:
        f.write(line + "\n")
print(line)
