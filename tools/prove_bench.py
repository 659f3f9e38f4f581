"""Proofs per second of lsr_r1cs_prove_batch_device and lsr_r1cs_verify_batch_device (device events), against the same proofs made by
chaining the existing entry points with host evaluation.  One JSON line per configuration.

    python tools/prove_bench.py --m 4096 --batch 4096 [--zk] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402

Q = 18446744069414584321
CQ = 17592186044417


def circuit(m, free_vars=4):
    """(A_i z)(B_i z) = z[free + i] with two entries per row of A and B: the witness of any free assignment is cheap to extend"""
    rng = np.random.default_rng(m)
    a, b, c = [], [], []
    for i in range(m):
        for mat in (a, b):
            for col in rng.choice(free_vars + i, size=min(2, free_vars + i), replace=False):
                mat.append((i, int(col), int(rng.integers(1, Q, dtype=np.uint64))))
        c.append((i, free_vars + i, 1))
    return free_vars + m, a, b, c


def witnesses(m, n, a, b, batch, free_vars=4):
    rng = np.random.default_rng(7)
    ra, rb = [[] for _ in range(m)], [[] for _ in range(m)]
    for (i, col, v) in a: ra[i].append((col, v))
    for (i, col, v) in b: rb[i].append((col, v))
    ws = np.zeros((batch, n), dtype=np.uint64)
    ws[:, :free_vars] = rng.integers(0, Q, size=(batch, free_vars), dtype=np.uint64)
    z = [[int(x) for x in row] for row in ws[:, :free_vars]]
    for s in range(batch):
        zs = z[s] + [0] * m
        for i in range(m):
            zs[free_vars + i] = (sum(v * zs[col] for col, v in ra[i]) % Q) * (sum(v * zs[col] for col, v in rb[i]) % Q) % Q
        ws[s] = zs
    return ws


def timed(fn, reps):
    s = torch.cuda.current_stream()
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    best = []
    for _ in range(reps):
        ev[0].record(s); fn(); ev[1].record(s)
        torch.cuda.synchronize()
        best.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(best))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--zk", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chain-sample", type=int, default=8, help="proofs whose host evaluation is timed for the chained comparison")
    args = ap.parse_args()
    pkg = entry.load_package()
    m, batch, n_public = args.m, args.batch, 2
    n, a, b, c = circuit(m)
    base = witnesses(m, n, a, b, min(batch, 64))
    ws = np.concatenate([base] * ((batch + 63) // 64))[:batch]
    ctx = pkg.LweContext(pkg.Params(q=CQ, n=4096, k=2, sigma=3.19), key_seed=0x5EED)
    prover = pkg.R1csProver(m, n, a, b, c)
    W = ctx.commitment_words
    seeds = np.arange(1, batch + 1, dtype=np.uint64)
    dw = torch.from_numpy(ws.view(np.int64)).cuda()
    blind = torch.from_numpy(np.arange(batch, dtype=np.uint64).view(np.int64) * 977).cuda() if args.zk else None
    drows = torch.zeros((batch, W), dtype=torch.int64, device="cuda")
    dproofs = torch.zeros((batch, 13), dtype=torch.int64, device="cuda")
    dhash = torch.zeros((batch, 64), dtype=torch.uint8, device="cuda")
    dstat = torch.zeros(batch, dtype=torch.int32, device="cuda")
    dres = torch.zeros(batch, dtype=torch.int32, device="cuda")
    dpub = dw[:, :n_public].contiguous()
    s = torch.cuda.current_stream().cuda_stream

    def prove():
        prover.prove_batch_device(ctx, dw.data_ptr(), batch, seeds, n_public, ctx.modulus(), drows.data_ptr(), dproofs.data_ptr(), dhash.data_ptr(),
                                  dstat.data_ptr(), None if blind is None else blind.data_ptr(), s)

    def verify():
        pkg.verify_r1cs_batch_device(m, dpub.data_ptr(), n_public, drows.data_ptr(), W, dproofs.data_ptr(), batch, dres.data_ptr(), zk=args.zk, stream=s)

    prove_ms = timed(prove, args.reps)
    verify_ms = timed(verify, args.reps)
    ok = int((dres.cpu().numpy() == 1).sum())
    # the chain: quotient -> commitment rows -> two transcripts on the device entry points, then host interpolation and evaluation
    t0 = time.perf_counter()
    quot, lens = prover.quotient_batch(ws)
    rows = pkg.Commitment.batch_words(ctx, quot % np.uint64(CQ), seeds)
    alphas = np.zeros(batch, dtype=np.uint64); betas = np.zeros(batch, dtype=np.uint64)
    pub = np.ascontiguousarray(ws[:, :n_public])
    lib = pkg._abi.lib()
    lib.lsr_fs_challenge_batch_flat(pub.ctypes.data, n_public, rows.ctypes.data, W, batch, Q, alphas.ctypes.data, None, 0)
    lib.lsr_fs_challenge_batch_flat(alphas.ctypes.data, 1, rows.ctypes.data, W, batch, Q, betas.ctypes.data, None, 0)
    chain_device_s = time.perf_counter() - t0
    oracle = entry.load_oracle()
    omega = oracle.prover_omega(m)
    ea, eb, ec = prover.compute_constraint_evals(ws[:args.chain_sample])
    t0 = time.perf_counter()
    for i in range(args.chain_sample):
        polys = [oracle.cyclic_inverse(v[i], Q, omega) for v in (ea, eb, ec)] + [quot[i, :lens[i]]]
        for p in polys:
            for x in (int(alphas[i]), int(betas[i])):
                oracle.eval_poly(p, x, Q)
    host_eval_s = (time.perf_counter() - t0) / args.chain_sample * batch
    print(json.dumps({"m": m, "batch": batch, "zk": args.zk, "prove_ms": round(prove_ms, 3), "prove_proofs_per_s": round(batch / prove_ms * 1e3, 1),
                      "verify_ms": round(verify_ms, 3), "verify_proofs_per_s": round(batch / verify_ms * 1e3, 1), "verified": ok,
                      "chain_device_steps_s": round(chain_device_s, 3), "chain_host_eval_s_extrapolated": round(host_eval_s, 3),
                      "chain_proofs_per_s": round(batch / (chain_device_s + host_eval_s), 1),
                      "rows_equal_chain": bool(np.array_equal(drows.cpu().numpy().view(np.uint64), rows))}))


if __name__ == "__main__":
    main()
