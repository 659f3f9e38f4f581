"""Seeded ring sampling on the device (lsr_ntt_ring_sample_batch_device, lsr_ntt_ring_matrix_create_seeded), all legs in one
process, alternating after a warm-up.  Prints ONE JSON line.

  (1) UNIFORM (exact, rejection) against the library's biased uniform_kernel (floor(word * q / 2^64), lsr_sampler.hip) on the same
      streams: q = 17592169062401, n = 4096, count = 16384 — 512 MiB of residues.  The biased kernel has no C entry point; it is
      driven through lsr::launch_uniform, found in the library's dynamic symbol table by name (uniform_harness below).  The two do
      the same cipher work; the fast paths differ by a compare and a wave-uniform branch against a multiply-high.  Criterion: the
      exact sampler's median is no more than 5 % plus the two spreads (max - min) above the biased kernel's.  The cipher-alone rate
      of tools/bin/ubench_sampler (`make -C tools bin/ubench_sampler`) is recorded beside them when that program is present.
  (2) BOUNDED at beta = 1 and BALL at kappa = 60, same q, n and count: recorded, nothing to compare with.
  (3) lsr_ntt_ring_matrix_create_seeded against lsr_ntt_ring_matrix_create from a ready (page-locked) host matrix, rows 64 x cols 256
      x n 4096 (512 MiB): wall-clock of the call, which is complete on return; the host matrix is generated outside the timed region.
      Criterion: the seeded call's median + spread below the host call's median.
env REPS (default 20), WARMUP (2), OUT (a JSON file to write, with the provenance stamp)."""
import ctypes
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import __graft_entry__ as entry  # noqa: E402
import provenance  # noqa: E402

Q, N, COUNT = 17592169062401, 4096, 16384
ROWS, COLS = 64, 256
UBENCH = os.path.join(ROOT, "tools", "bin", "ubench_sampler")


def uniform_harness(pkg):
    """lsr::launch_uniform(out, d_keys, index_base, components, domain, samples, objects, q, stream) of the loaded library."""
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg._abi.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    names = [line.split()[-1] for line in nm.splitlines() if "launch_uniform" in line]
    assert len(names) == 1, names
    fn = getattr(ctypes.CDLL(pkg._abi.LIB_PATH), names[0])
    fn.restype = None
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64,
                   ctypes.c_uint64, ctypes.c_void_p]
    return fn


def stats(times_us, out_bytes=None):
    row = {"us_median": round(float(np.median(times_us)), 1), "us_min": round(float(np.min(times_us)), 1), "us_max": round(float(np.max(times_us)), 1),
           "us_spread": round(float(np.max(times_us) - np.min(times_us)), 1)}
    if out_bytes:
        row["gb_per_s"] = round(out_bytes / row["us_median"] / 1e3, 1)
        row["g_coefficients_per_s"] = round(out_bytes / 8 / row["us_median"] / 1e3, 2)
    return row


def alternate(legs, reps, warmup):
    for _ in range(1 + warmup):
        for _, fn in legs:
            fn()
    torch.cuda.synchronize()
    times = {key: [] for key, _ in legs}
    for _ in range(reps):
        for key, fn in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[key].append(e0.elapsed_time(e1) * 1e3)
    return times


def sampling_legs(pkg, biased, reps, warmup):
    ctx = pkg.NttContext(Q, N, device=0)
    s = torch.cuda.current_stream().cuda_stream
    key = torch.from_numpy(pkg.ring_sample_key(1).view(np.int64)).cuda()
    out = torch.empty((COUNT, N), dtype=torch.int64, device="cuda")

    def sample(kind, param):
        return lambda: ctx.ring_sample_device(out.data_ptr(), COUNT, kind, param, key.data_ptr(), COUNT, stream=s)
    legs = (("uniform_exact", sample(pkg.RING_SAMPLE_UNIFORM, 0)),
            ("uniform_biased", lambda: biased(out.data_ptr(), key.data_ptr(), 0, COUNT, 16, N, COUNT, Q, s)),
            ("bounded_beta1", sample(pkg.RING_SAMPLE_BOUNDED, 1)), ("ball_kappa60", sample(pkg.RING_SAMPLE_BALL, 60)))
    times = alternate(legs, reps, warmup)
    ctx.close()
    rows = {k: stats(t, COUNT * N * 8) for k, t in times.items()}
    e, b = rows["uniform_exact"], rows["uniform_biased"]
    rows["exact_over_biased"] = round(e["us_median"] / b["us_median"], 3)
    rows["bound_us"] = round(b["us_median"] * 1.05 + e["us_spread"] + b["us_spread"], 1)
    rows["exact_within_5_percent_plus_spreads"] = bool(e["us_median"] <= rows["bound_us"])
    return rows


def cipher_alone():
    """The best 'cipher only' line of ubench_sampler: G samples (64-bit words) per second, or None when the program is not built."""
    if not os.path.exists(UBENCH):
        return None
    text = subprocess.run([UBENCH], stdout=subprocess.PIPE, text=True, timeout=300).stdout
    rates = [float(m.group(1)) for m in re.finditer(r"cipher only[^\n]*?([0-9.]+) G units/s", text)]
    return max(rates) if rates else None


def matrix_legs(pkg, reps, warmup):
    ctx = pkg.NttContext(Q, N, device=0)
    host = pkg.PinnedArray((ROWS, COLS, N))
    host.array[...] = np.random.default_rng(1).integers(0, Q, size=(ROWS, COLS, N), dtype=np.uint64)
    key = pkg.ring_sample_key(1)
    lib = ctx._lib

    def timed(make):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        handle = make()
        dt = (time.perf_counter() - t0) * 1e6
        assert handle, pkg._abi.last_error()
        lib.lsr_ntt_ring_matrix_free(handle)
        return dt
    legs = (("create_seeded", lambda: lib.lsr_ntt_ring_matrix_create_seeded(ctx.handle, key.ctypes.data, 16, 0, ROWS, COLS)),
            ("create_from_host", lambda: lib.lsr_ntt_ring_matrix_create(ctx.handle, host.ptr, ROWS, COLS)))
    times = {k: [] for k, _ in legs}
    for rep in range(warmup + reps):
        for k, make in legs:
            dt = timed(make)
            if rep >= warmup:
                times[k].append(dt)
    host.close()
    ctx.close()
    rows = {k: stats(t) for k, t in times.items()}
    rows["matrix_bytes"] = ROWS * COLS * N * 8
    rows["host_over_seeded"] = round(rows["create_from_host"]["us_median"] / rows["create_seeded"]["us_median"], 2)
    rows["seeded_median_plus_spread_below_host_median"] = bool(rows["create_seeded"]["us_median"] + rows["create_seeded"]["us_spread"]
                                                               < rows["create_from_host"]["us_median"])
    return rows


def main():
    reps, warmup = int(os.environ.get("REPS", "20")), int(os.environ.get("WARMUP", "2"))
    pkg = entry.load_package()
    # the child processes run before this process opens the GPU
    cipher, biased = cipher_alone(), uniform_harness(pkg)
    out = {"tool": "ring_sample_bench", "reps": reps, "warmup": warmup, "q": Q, "n": N, "count": COUNT,
           "sampling": sampling_legs(pkg, biased, reps, warmup)}
    torch.cuda.empty_cache()
    out["matrix"] = matrix_legs(pkg, reps, warmup)
    out["cipher_alone_g_words_per_s"] = cipher
    out["provenance"] = provenance.provenance()
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
