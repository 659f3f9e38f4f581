"""Proofs per second of lsr_simple_prove_batch_device (prove_simple / prove_zk) and lsr_simple_verify_batch_device (verify_simple) at
n = 4096, k = 2, plus the coefficient rate of lsr_random_blinding_device beside lsr_random_blinding on one host core.
One JSON line per (mode, L), then one for random_blinding.

    python tools/simple_prove_bench.py [--lengths 4 64 1024 4096] [--batch 4096] [--modes plain zk] [--reps 5] [--out FILE]
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
import __graft_entry__ as entry  # noqa: E402

CQ = 17592186044417                     # Params.q = Rust's LweContext::modulus(); also the field modulus here


def timed(fn, reps):
    s = torch.cuda.current_stream()
    fn()                                # warm-up: workspace allocation, first launches
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = []
    for _ in range(reps):
        ev[0].record(s); fn(); ev[1].record(s)
        torch.cuda.synchronize()
        out.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(out))


def run(pkg, ctx, prover, mode, length, batch, reps):
    rng = np.random.default_rng(length)
    W, n_public = ctx.commitment_words, 2
    seeds = np.arange(1, batch + 1, dtype=np.uint64)
    dw = torch.from_numpy(rng.integers(0, 2**64, size=(batch, length), dtype=np.uint64).view(np.int64)).cuda()
    dpub = torch.from_numpy(rng.integers(0, 2**64, size=(batch, n_public), dtype=np.uint64).view(np.int64)).cuda()
    dkeys = torch.from_numpy(pkg.chacha20rng_keys(np.arange(batch, dtype=np.uint64) + 7).view(np.int64)).cuda() if mode != "plain" else None
    drows = torch.zeros((batch, W), dtype=torch.int64, device="cuda")
    dco = torch.zeros((batch, length), dtype=torch.int64, device="cuda")
    dpr = torch.zeros((batch, 3), dtype=torch.int64, device="cuda")
    dres = torch.zeros(batch, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def prove():
        prover.prove_batch_device(ctx, dw.data_ptr(), length, batch, dpub.data_ptr(), n_public, seeds, ctx.modulus(), drows.data_ptr(), dco.data_ptr(),
                                  dpr.data_ptr(), mode=mode, d_blinding_keys=None if dkeys is None else dkeys.data_ptr(), stream=s)

    def verify():
        pkg.verify_simple_batch_device(prover.modulus, dpub.data_ptr(), n_public, drows.data_ptr(), W, dpr.data_ptr(), dco.data_ptr(), length, batch,
                                       dres.data_ptr(), stream=s)

    prove_ms = timed(prove, reps)
    verify_ms = timed(verify, reps)
    ok = int((dres.cpu().numpy() == 1).sum())
    return {"mode": mode, "length": length, "batch": batch, "q": prover.modulus, "n": 4096, "k": 2, "prove_ms": round(prove_ms, 3),
            "prove_proofs_per_s": round(batch / prove_ms * 1e3, 1), "verify_ms": round(verify_ms, 3),
            "verify_proofs_per_s": round(batch / verify_ms * 1e3, 1), "verified": ok}


def blinding_rate(pkg, batch, length, q, reps):
    keys = pkg.chacha20rng_keys(np.arange(batch, dtype=np.uint64))
    dk = torch.from_numpy(keys.view(np.int64)).cuda()
    out = torch.zeros((batch, length), dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    dev_ms = timed(lambda: pkg.random_blinding_device(dk.data_ptr(), batch, length, q, out.data_ptr(), s), reps)
    host_batch = max(1, batch // 16)
    t0 = time.perf_counter()
    host = pkg.random_blinding(keys[:host_batch], length, q)      # one thread
    host_s = time.perf_counter() - t0
    same = bool(np.array_equal(out[:host_batch].cpu().numpy().view(np.uint64), host))
    return {"what": "random_blinding", "batch": batch, "length": length, "q": q, "device_ms": round(dev_ms, 3),
            "device_gcoeffs_per_s": round(batch * length / dev_ms / 1e6, 2), "host_one_core_gcoeffs_per_s": round(host_batch * length / host_s / 1e9, 4),
            "host_rows_timed": host_batch, "device_equals_host": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lengths", type=int, nargs="+", default=[4, 64, 1024, 4096])
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--modes", nargs="+", default=["plain", "zk"])
    ap.add_argument("--q", type=int, default=CQ)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-blinding", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = entry.load_package()
    ctx = pkg.LweContext(pkg.Params(q=CQ, n=4096, k=2, sigma=3.19), key_seed=0x5EED)
    prover = pkg.SimpleProver(args.q)
    lines = []
    for mode in args.modes:
        for length in args.lengths:
            lines.append(run(pkg, ctx, prover, mode, length, args.batch, args.reps))
            print(json.dumps(lines[-1]), flush=True)
    if not args.no_blinding:
        lines.append(blinding_rate(pkg, args.batch, 4096, args.q, args.reps))
        print(json.dumps(lines[-1]), flush=True)
    prover.close()
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
