"""Measurements of the 2^18 .. 2^22 sizes of the NTT path: device events, median of the repetitions, one JSON line
per shape.

    python tools/large_circuit_bench.py transform --logn 17 18 20 22 [--gib 2] [--lib PATH]   # cyclic forward, time per residue
    python tools/large_circuit_bench.py eval --logm 20 --batch 4                             # evaluation of A, B, C, Q at two points
    python tools/large_circuit_bench.py prove --logm 18 --batch 16                           # lsr_r1cs_prove_batch_device, whole call
    python tools/large_circuit_bench.py oracle --logm 18                                     # the oracle's sequence for ONE proof, one core, no GPU

`transform --lib PATH` binds the named build of the library through its C-ABI alone (sizes <= 2^17 exist in every build), so the same
tool times another commit's library on the same machine.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402

Q = 18446744069414584321
CQ = 17592186044417
FREE = 8


def timed(torch, fn, reps):
    s = torch.cuda.current_stream()
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = []
    for _ in range(reps):
        ev[0].record(s); fn(); ev[1].record(s)
        torch.cuda.synchronize()
        out.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(out)), out


def cmd_transform(args):
    import torch
    pkg = entry.load_package()
    pkg._abi._share_hip_runtime_with_torch()
    path = args.lib or pkg._abi.LIB_PATH
    lib = ctypes.CDLL(path)
    u64, u32, vp, ci, sz = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    lib.lsr_ntt_forward_batch_device.restype = ci
    lib.lsr_ntt_forward_batch_device.argtypes = [vp, vp, sz, vp]
    lib.ntt_context_free.argtypes = [vp]
    for logn in args.logn:
        n = 1 << logn
        create = getattr(lib, "lsr_cyclic_ntt_context_create_large" if logn > 17 else "lsr_cyclic_ntt_context_create")
        create.restype, create.argtypes = vp, [u64, u32, u64, ci]
        h = create(Q, n, 0, -1)
        if not h:
            raise SystemExit(f"no context for n = 2^{logn} in {path}")
        batch = max(1, int(args.gib * (1 << 30)) // (n * 8))
        d = torch.randint(0, 2**62, (batch, n), dtype=torch.int64, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        ms, all_ms = timed(torch, lambda: lib.lsr_ntt_forward_batch_device(h, d.data_ptr(), batch, s), args.reps)
        lib.ntt_context_free(h)
        del d
        print(json.dumps({"what": "cyclic_forward_device", "lib": os.path.basename(path), "logn": logn, "batch": batch, "gib": round(batch * n * 8 / 2**30, 3),
                          "ms": round(ms, 3), "ns_per_residue": round(ms * 1e6 / (batch * n), 5), "reps_ms": [round(v, 3) for v in all_ms]}), flush=True)


def cmd_eval(args):
    import torch
    pkg = entry.load_package()
    for logm in args.logm:
        m, polys = 1 << logm, 4 * args.batch                         # A, B, C, Q of `batch` instances, each at alpha and beta
        c = torch.randint(0, 2**62, (polys, m), dtype=torch.int64, device="cuda")
        x = torch.randint(0, 2**62, (polys, 2), dtype=torch.int64, device="cuda")
        v = torch.zeros((polys, 2), dtype=torch.int64, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        ms, all_ms = timed(torch, lambda: pkg.prover_eval_batch_device(c.data_ptr(), m, polys, x.data_ptr(), 2, v.data_ptr(), s), args.reps)
        print(json.dumps({"what": "eval_batch_device", "logm": logm, "instances": args.batch, "polys": polys, "points": 2, "ms": round(ms, 4),
                          "bytes": polys * m * 8, "tb_per_s": round(polys * m * 8 / (ms * 1e-3) / 1e12, 3), "reps_ms": [round(t, 4) for t in all_ms]}),
              flush=True)


def make_case(oracle, logm, batch):
    from test_large_circuit_abi import build_circuit, make_witness
    m = 1 << logm
    rng = np.random.default_rng(1000 + logm)
    n, mats = build_circuit(rng, m, free_vars=FREE)
    base = make_witness(oracle, rng.integers(0, 2**64, size=FREE, dtype=np.uint64), m, mats)
    return m, n, mats, np.stack([base] * batch)


def cmd_prove(args):
    import torch
    pkg = entry.load_package()
    oracle = entry.load_oracle()
    ctx = pkg.LweContext(pkg.Params(q=CQ, n=4096, k=2, sigma=3.19), key_seed=0x5EED)
    for logm in args.logm:
        m, n, mats, ws = make_case(oracle, logm, args.batch)
        batch, n_public = args.batch, 2
        prover = pkg.R1csProver(m, n, *mats)
        W = ctx.commitment_words
        seeds = np.arange(1, batch + 1, dtype=np.uint64)
        dw = torch.from_numpy(ws.view(np.int64)).cuda()
        drows = torch.zeros((batch, W), dtype=torch.int64, device="cuda")
        dproofs = torch.zeros((batch, 13), dtype=torch.int64, device="cuda")
        dstat = torch.zeros(batch, dtype=torch.int32, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        ms, all_ms = timed(torch, lambda: prover.prove_batch_device(ctx, dw.data_ptr(), batch, seeds, n_public, ctx.modulus(), drows.data_ptr(),
                                                                     dproofs.data_ptr(), 0, dstat.data_ptr(), None, s), args.reps)
        ok = pkg.verify_r1cs_batch(m, ws[:, :n_public], drows.cpu().numpy().view(np.uint64), dproofs.cpu().numpy().view(np.uint64))
        prover.close()
        print(json.dumps({"what": "r1cs_prove_batch_device", "logm": logm, "batch": batch, "ms": round(ms, 3), "ms_per_proof": round(ms / batch, 3),
                          "verified": int(ok.sum()), "status_min": int(dstat.cpu().numpy().min()), "reps_ms": [round(t, 3) for t in all_ms]}), flush=True)
    ctx.close()


def cmd_oracle(args):
    """sparse products, quotient (transforms of size m and 2m), and the eight evaluations of one proof on one CPU core"""
    from test_large_circuit_abi import fast_quotient, sparse_mul_vec
    oracle = entry.load_oracle()
    for logm in args.logm:
        m, n, mats, ws = make_case(oracle, logm, 1)
        t0 = time.perf_counter()
        evals = [sparse_mul_vec(oracle, mat, m, ws[0]) for mat in mats]
        quot, ln, polys = fast_quotient(oracle, *evals)
        for poly in polys + (quot[:ln],):
            for x in (0x1234567890ABCDEF % Q, 0xFEDCBA0987654321 % Q):
                oracle.eval_poly(poly, x, Q)
        print(json.dumps({"what": "oracle_sequence_one_proof_one_core", "logm": logm, "s": round(time.perf_counter() - t0, 2), "quotient_len": ln}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("transform"); t.add_argument("--logn", type=int, nargs="+", default=[18, 20, 22]); t.add_argument("--gib", type=float, default=2.0)
    t.add_argument("--lib", default=None); t.add_argument("--reps", type=int, default=7); t.set_defaults(fn=cmd_transform)
    e = sub.add_parser("eval"); e.add_argument("--logm", type=int, nargs="+", default=[20]); e.add_argument("--batch", type=int, default=4)
    e.add_argument("--reps", type=int, default=9); e.set_defaults(fn=cmd_eval)
    p = sub.add_parser("prove"); p.add_argument("--logm", type=int, nargs="+", default=[18]); p.add_argument("--batch", type=int, default=16)
    p.add_argument("--reps", type=int, default=3); p.set_defaults(fn=cmd_prove)
    o = sub.add_parser("oracle"); o.add_argument("--logm", type=int, nargs="+", default=[18]); o.set_defaults(fn=cmd_oracle)
    args = ap.parse_args()
    args.fn(args)


if __name__ == "__main__":
    main()
