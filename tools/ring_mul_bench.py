"""Fused ring multiply (lsr_ntt_ring_mul_batch_device) against the composed sequence a caller would otherwise chain — copies of a and b
(the transforms work in place), forward, forward, pointwise product, inverse — on the same seeded device-resident inputs, in one
process, the two schedules alternating after a warm-up.  Prints ONE JSON line.

  n = 4096 at q = 17592169062401 (north_star's prime), 65,536 products; n = 2^16 at q = 17592182243329, 512 products;
  b_rows = batch and b_rows = 1 at both sizes.

Composed form with b_rows = 1: b is copied and transformed once, its transform repeated over the batch (ntt_mul_pointwise takes
[count] operands), then pointwise and inverse.  Bytes per output residue are computed from the shapes (8 bytes per word read or
written in HBM; a transform is one pass of read + write per kernel: 1 kernel at n <= 4096, 2 above).
env REPS (default 10), WARMUP (default 2)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import __graft_entry__ as entry  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
CONFIGS = [(17592169062401, 4096, 65536), (17592182243329, 65536, 512)]


def bytes_per_residue(n, shared):
    passes = 1 if n <= 4096 else 2          # kernels per transform, each reads and writes the array once
    t = 16 * passes
    if shared:
        fused = 16 if n <= 4096 else 16 + 16 + 16          # n > 4096: strided a -> c, middle (c in place; b-hat L2-resident), strided inverse
        composed = 16 + t + 8 + 24 + t                     # copy a, forward a, repeat b-hat, pointwise, inverse
    else:
        fused = 24 if n <= 4096 else 16 + 16 + 24 + 16     # b -> workspace, a -> c, middle (c, workspace -> c), strided inverse
        composed = 16 + 16 + t + t + 24 + t                # copy a, copy b, forward a, forward b, pointwise, inverse
    return fused, composed


def main():
    reps, warmup = int(os.environ.get("REPS", "10")), int(os.environ.get("WARMUP", "2"))
    pkg = entry.load_package()
    results = []
    for q, n, batch in CONFIGS:
        ctx = pkg.NttContext(q, n, device=0)
        g = torch.Generator(device="cuda")
        g.manual_seed(n)
        a = torch.randint(0, q, (batch, n), dtype=torch.int64, device="cuda", generator=g)
        b_full = torch.randint(0, q, (batch, n), dtype=torch.int64, device="cuda", generator=g)
        c_fused = torch.empty_like(a)
        ta, tb, c_comp = torch.empty_like(a), torch.empty_like(a), torch.empty_like(a)
        s = torch.cuda.current_stream().cuda_stream
        for shared in (False, True):
            b = b_full[:1] if shared else b_full
            b_rows = 1 if shared else batch
            b1 = torch.empty_like(b_full[:1])

            def fused():
                ctx.ring_mul_device(c_fused.data_ptr(), a.data_ptr(), b.data_ptr(), batch, b_rows, s)

            def composed():
                ta.copy_(a)
                ctx.forward_device(ta.data_ptr(), batch, s)
                if shared:
                    b1.copy_(b)
                    ctx.forward_device(b1.data_ptr(), 1, s)
                    tb.copy_(b1.expand(batch, n))
                else:
                    tb.copy_(b)
                    ctx.forward_device(tb.data_ptr(), batch, s)
                ctx.mul_pointwise_device(c_comp.data_ptr(), ta.data_ptr(), tb.data_ptr(), batch * n, s)
                ctx.inverse_device(c_comp.data_ptr(), batch, s)

            for _ in range(warmup):
                fused()
                composed()
            torch.cuda.synchronize()
            times = {"fused": [], "composed": []}
            for _ in range(reps):
                for name, fn in (("fused", fused), ("composed", composed)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    times[name].append(e0.elapsed_time(e1) * 1e3)
            equal = bool(torch.equal(c_fused, c_comp))
            fb, cb = bytes_per_residue(n, shared)
            row = {"n": n, "q": q, "batch": batch, "b_rows": b_rows, "outputs_equal": equal, "bytes_per_residue": {"fused": fb, "composed": cb}}
            for name in ("fused", "composed"):
                us = float(np.median(times[name]))
                row[name] = {"us_per_call": round(us, 1), "us_min": round(float(np.min(times[name])), 1),
                             "products_per_s": round(batch / (us * 1e-6)), "roofline_fraction_at_24B": round(24 * batch * n / (us * 1e-6) / HBM_BYTES_PER_S, 3)}
            row["speedup"] = round(row["composed"]["us_per_call"] / row["fused"]["us_per_call"], 2)
            results.append(row)
        del a, b_full, c_fused, ta, tb, c_comp
        ctx.close()
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "ring_mul_bench", "reps": reps, "warmup": warmup, "configs": results,
                      "all_equal": all(r["outputs_equal"] for r in results)}))


if __name__ == "__main__":
    main()
