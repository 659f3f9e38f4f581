"""Proofs per second of lsr_r1cs_prove_batch_device and lsr_r1cs_verify_batch_mod_device on the Lagrange path, with
the interpolation GEMM's modular-MAC rate from its share of the kernel time when run under rocprofv3.  One JSON line per m.

    python tools/lagrange_prove_bench.py --m 10 20 30 32 --batch 4096 [--q 17592186044423] [--zk] [--reps 5]

The reference's published prove_r1cs latencies (4.45 ms at m = 10, 389 us at m = 32, hardware unstated) are one proof
at a time on a CPU; they are printed beside the batch rate for orientation only.
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
import lagrange_oracle as lo  # noqa: E402

CQ = 17592186044417
REFERENCE_US = {10: 4450.0, 32: 389.0}     # BASELINE.md §2, one proof, hardware unstated


def timed(fn, reps):
    s = torch.cuda.current_stream()
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = []
    for _ in range(reps):
        ev[0].record(s); fn(); ev[1].record(s)
        torch.cuda.synchronize()
        out.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(out))


def run(pkg, ctx, m, q, batch, zk, reps):
    rng = np.random.default_rng(m)
    n, a, b, c = lo.random_circuit(rng, m, 4, q)
    base = np.stack([lo.extend_witness(rng.integers(0, 2**64, size=4, dtype=np.uint64), m, a, b, q) for _ in range(min(batch, 16))])
    ws = np.concatenate([base] * ((batch + len(base) - 1) // len(base)))[:batch]
    t0 = time.perf_counter()
    prover = pkg.R1csProver(m, n, a, b, c, modulus=q)
    create_s = time.perf_counter() - t0
    W, n_public = ctx.commitment_words, 2
    seeds = np.arange(1, batch + 1, dtype=np.uint64)
    dw = torch.from_numpy(ws.view(np.int64)).cuda()
    blind = torch.from_numpy(np.arange(batch, dtype=np.uint64).view(np.int64) * 977).cuda() if zk else None
    drows = torch.zeros((batch, W), dtype=torch.int64, device="cuda")
    dproofs = torch.zeros((batch, 13), dtype=torch.int64, device="cuda")
    dstat = torch.zeros(batch, dtype=torch.int32, device="cuda")
    dres = torch.zeros(batch, dtype=torch.int32, device="cuda")
    dpub = dw[:, :n_public].contiguous()
    s = torch.cuda.current_stream().cuda_stream

    def prove():
        prover.prove_batch_device(ctx, dw.data_ptr(), batch, seeds, n_public, ctx.modulus(), drows.data_ptr(), dproofs.data_ptr(), 0, dstat.data_ptr(),
                                  None if blind is None else blind.data_ptr(), s)

    def verify():
        pkg.verify_r1cs_batch_device(m, dpub.data_ptr(), n_public, drows.data_ptr(), W, dproofs.data_ptr(), batch, dres.data_ptr(), zk=zk, stream=s,
                                     modulus=q)

    prove_ms = timed(prove, reps)
    verify_ms = timed(verify, reps)
    ok = int((dres.cpu().numpy() == 1).sum())
    proved = int((dstat.cpu().numpy() > 0).sum())
    prover.close()
    rec = {"m": m, "q": q, "batch": batch, "zk": zk, "create_s": round(create_s, 3), "prove_ms": round(prove_ms, 3),
           "prove_proofs_per_s": round(batch / prove_ms * 1e3, 1), "prove_us_per_proof": round(prove_ms * 1e3 / batch, 3),
           "verify_ms": round(verify_ms, 3), "verify_proofs_per_s": round(batch / verify_ms * 1e3, 1), "proved": proved, "verified": ok,
           "gemm_macs": 3 * batch * m * m}
    if m in REFERENCE_US:
        rec["reference_prove_us_per_proof_hardware_unstated"] = REFERENCE_US[m]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, nargs="+", default=[10, 20, 30, 32])
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--q", type=int, default=17592186044423)
    ap.add_argument("--zk", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    pkg = entry.load_package()
    ctx = pkg.LweContext(pkg.Params(q=CQ, n=4096, k=2, sigma=3.19), key_seed=0x5EED)
    for m in args.m:
        print(json.dumps(run(pkg, ctx, m, args.q, args.batch, args.zk, args.reps)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
