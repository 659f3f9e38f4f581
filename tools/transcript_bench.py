"""Fiat–Shamir transcript throughput over reference-size commitments (12 293-word, 98 KB rows).

  --host     lsr_fs_challenge_batch_flat over 2048 rows on 1 .. 32 host threads (text lines).
  --device   (default) the device sweep: counts {1, 8, 64, 512, 2048, 4096, 8192, 16 384, 32 768, 65 536}, the lane kernel (LANE) and
             the wavefront-cooperative kernel (WAVE) — with --auto also what lsr_fs_transcript_path picks (AUTO) — single challenge and
             the chained alpha -> beta pair, device events, WARMUP (2) warm-ups and the median of REPS (10) calls with the paths
             alternating inside every repeat in an order that rotates from repeat to repeat (at 65 536 rows the lane kernel takes
             17.6 ms instead of 10.7 when it follows the 100 ms wave kernel, whichever name it runs under); the outputs of the paths
             are compared in every configuration.  Prints ONE JSON line with
             the provenance stamp of tools/provenance.py.
  --counts 1,64,...      another list of counts.
  --paths lane,auto      another set of paths to alternate.
  --entry-only           time only the plain lsr_fs_challenge_batch_device entry (any build has it) — with --library PATH this is how
                         an older build of the library is timed next to this one, in a process of its own."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import __graft_entry__ as entry  # noqa: E402
import provenance  # noqa: E402

W, Q = 12293, 17592186044417
COUNTS = [1, 8, 64, 512, 2048, 4096, 8192, 16384, 32768, 65536]
PATHS = {"auto": 0, "lane": 1, "wave": 2}


def host_sweep(lib):
    count = 2048
    rows = np.random.default_rng(1).integers(0, 2**64, size=(count, W), dtype=np.uint64)
    al = np.zeros(count, dtype=np.uint64)
    for th in (1, 2, 4, 8, 16, 32):
        t = time.perf_counter()
        assert lib.lsr_fs_challenge_batch_flat(None, 0, rows.ctypes.data, W, count, Q, al.ctypes.data, None, th) == 0
        dt = time.perf_counter() - t
        print(f"{th:2d} threads: {dt*1e3:7.1f} ms = {count/dt/1e3:6.1f} K transcripts/s, {count*W*8/dt/1e9:5.2f} GB/s", flush=True)


def timed(torch, fns, reps, warmup):
    """fns: name -> callable enqueueing one call on the current stream.  Alternating calls, one pair of events per call; microseconds."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    order = list(fns)
    for rep in range(reps):
        for name in order[rep % len(order):] + order[:rep % len(order)]:      # every path follows every other one equally often
            fn = fns[name]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3)
    return {name: {"us": round(float(np.median(t)), 1), "us_min": round(float(np.min(t)), 1), "us_max": round(float(np.max(t)), 1),
                   "spread_pct": round(100.0 * (float(np.max(t)) - float(np.min(t))) / float(np.median(t)), 1)} for name, t in times.items()}


def device_sweep(lib, counts, names, reps, warmup, entry_only):
    import torch
    s = torch.cuda.current_stream().cuda_stream
    top = max(counts)
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    rows = torch.randint(-2**63, 2**63 - 1, (top, W), dtype=torch.int64, device="cuda", generator=g)
    pub = torch.randint(0, Q, (top, 2), dtype=torch.int64, device="cuda", generator=g)
    out = {n: {k: torch.zeros(top, dtype=torch.int64, device="cuda") for k in ("a1", "a", "b")} for n in names}
    results = []
    for count in counts:
        row = {"count": count}
        if entry_only:
            o = out[names[0]]
            fns = {"entry": lambda: lib.lsr_fs_challenge_batch_device(pub.data_ptr(), 2, rows.data_ptr(), W, count, Q, o["a1"].data_ptr(), None, s)}
            row["single"] = timed(torch, fns, reps, warmup)
            results.append(row)
            continue
        row["auto_picks"] = {1: "lane", 2: "wave"}[lib.lsr_fs_transcript_path(count, W)]
        single = {n: (lambda n=n: lib.lsr_fs_challenge_batch_device_on(PATHS[n], pub.data_ptr(), 2, rows.data_ptr(), W, count, Q,
                                                                        out[n]["a1"].data_ptr(), None, s)) for n in names}
        chain = {n: (lambda n=n: lib.lsr_fs_challenge_chain_batch_device(PATHS[n], pub.data_ptr(), 2, rows.data_ptr(), W, count, Q, out[n]["a"].data_ptr(),
                                                                          out[n]["b"].data_ptr(), None, None, s)) for n in names}
        row["single"] = timed(torch, single, reps, warmup)
        row["chain"] = timed(torch, chain, reps, warmup)
        ref = out[names[0]]
        row["outputs_equal"] = all(bool(torch.equal(out[n][k][:count], ref[k][:count])) for n in names for k in ("a1", "a", "b")) and \
            bool(torch.equal(ref["a1"][:count], ref["a"][:count]))
        if "lane" in names and "wave" in names:
            row["wave_speedup"] = {k: round(row[k]["lane"]["us"] / row[k]["wave"]["us"], 2) for k in ("single", "chain")}
        results.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--auto", action="store_true")
    ap.add_argument("--entry-only", action="store_true")
    ap.add_argument("--library")
    ap.add_argument("--counts")
    ap.add_argument("--paths", help="e.g. lane,auto: the paths to alternate (default lane,wave and, with --auto, auto)")
    args = ap.parse_args()
    pkg = entry.load_package()
    if args.library:
        pkg._abi._share_hip_runtime_with_torch()
        lib = ctypes.CDLL(args.library)      # an older build lacks the newer symbols: bind only what --entry-only calls
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        lib.lsr_fs_challenge_batch_device.argtypes = [vp, sz, vp, sz, sz, ctypes.c_uint64, vp, vp, vp]
        assert args.entry_only, "--library goes with --entry-only"
    else:
        lib = pkg._abi.lib()
    if args.host:
        host_sweep(lib)
    if args.device or not args.host:
        import torch
        assert torch.cuda.is_available(), "the device sweep needs a GPU"
        reps, warmup = int(os.environ.get("REPS", "10")), int(os.environ.get("WARMUP", "2"))
        counts = [int(c) for c in args.counts.split(",")] if args.counts else COUNTS
        names = args.paths.split(",") if args.paths else ["lane", "wave"] + (["auto"] if args.auto else [])
        results = device_sweep(lib, counts, names, reps, warmup, args.entry_only)
        stamp = provenance.provenance() if not args.library else {"library": os.path.basename(args.library), "lib_sha256": provenance.file_sha256(args.library)}
        print(json.dumps({"tool": "transcript_bench", "row_words": W, "n_inputs": 2, "reps": reps, "warmup": warmup, "device": torch.cuda.get_device_name(0),
                          "provenance": stamp, "configs": results,
                          "all_equal": all(r.get("outputs_equal", True) for r in results)}))


if __name__ == "__main__":
    main()
