"""Bit-packed ring elements (lsr_ntt_ring_pack_batch_device / lsr_ntt_ring_unpack_batch_device) against the only route the
library's users had: torch on the device.  One process, device-resident operands made by the library's own calls, the routes
alternating after a warm-up, HIP events, the outputs compared word for word at every shape.  Prints ONE JSON line.

  (a) pack / unpack:        ring_pack_device and ring_unpack_device.
  (b) torch_pack / torch_unpack: centre the words, make the shifted low and high part of every field and index_add_ them into the word
      array (the parts of one word have no bit in common, so the sum is the OR); back: two gathers, shifts, the sign extension and a
      masked q + v.  The index, shift and mask arrays depend on the shape alone and are built outside the timed region; the torch route
      computes no status and validates nothing.
  (c) l2sq: ring_l2sq_device over the same input buffer — the library's fastest pass over the same bytes, nothing written.
  (d) the host forms, wall clock, on pinned buffers, beside a plain device-to-pinned-host copy of the unpacked words (pack) and a
      pinned-host-to-device copy of them (unpack); and the route the codec exists for, where only packed words cross the bus: the
      device form followed by a copy of the packed words to pinned host memory, and that copy back up followed by the device unpack.

  Shapes, q = 17592182243329 (the FP64 flavour): n = 4096 x 16384 elements (512 MiB, past the Infinity Cache) —
  (A) bits = 11 CENTRED on ring_decompose digits of base 2^11;  (B) bits = 2 CENTRED on BALL elements;  (C) bits = 44 RESIDUE on UNIFORM
  elements;  (D) n = 64 x 2^20 elements at bits = 11 on digits.

env REPS (default 12), WARMUP (2), SHAPES (default "ABCD"), HOST_REPS (default 5), OUT (a JSON file to write, with the provenance stamp)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import __graft_entry__ as entry  # noqa: E402
import provenance  # noqa: E402
from ring_project_bench import timed  # noqa: E402

Q = 17592182243329
SHAPES = {"A": (4096, 16384, 11, 0, "digits"), "B": (4096, 16384, 2, 0, "ball"), "C": (4096, 16384, 44, 1, "uniform"), "D": (64, 1 << 20, 11, 0, "digits")}


def make_input(pkg, ctx, n, count, kind, s):
    out = torch.empty((count, n), dtype=torch.int64, device="cuda")
    key = torch.from_numpy(pkg.ring_sample_key(31).view(np.int64)).cuda()
    if kind == "digits":
        digits = pkg.ring_gadget_min_digits(Q, 11)
        sources = -(-count // digits)
        x = torch.empty((sources, n), dtype=torch.int64, device="cuda")
        out = torch.empty((sources * digits, n), dtype=torch.int64, device="cuda")
        ctx.ring_sample_device(x.data_ptr(), sources, pkg.RING_SAMPLE_UNIFORM, 0, key.data_ptr(), sources, stream=s)
        ctx.ring_decompose_device(out.data_ptr(), x.data_ptr(), sources, 11, digits, stream=s)
        out = out[:count]
    elif kind == "ball":
        ctx.ring_sample_device(out.data_ptr(), count, pkg.RING_SAMPLE_BALL, min(n, 60), key.data_ptr(), count, stream=s)
    else:
        ctx.ring_sample_device(out.data_ptr(), count, pkg.RING_SAMPLE_UNIFORM, 0, key.data_ptr(), count, stream=s)
    torch.cuda.synchronize()
    return out


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e6)
    return {"us_median": round(float(np.median(t)), 1), "us_min": round(float(np.min(t)), 1), "us_max": round(float(np.max(t)), 1),
            "us_spread": round(float(np.max(t) - np.min(t)), 1)}


def measure(pkg, name, reps, warmup, host_reps):
    n, count, bits, mode, kind = SHAPES[name]
    ctx = pkg.NttContext(Q, n, device=0)
    s = torch.cuda.current_stream().cuda_stream
    x = make_input(pkg, ctx, n, count, kind, s)
    total, wpe = count * n, pkg.ring_pack_words(n, bits)
    words, back = torch.empty((count, wpe), dtype=torch.int64, device="cuda"), torch.empty_like(x)
    status = torch.empty((2, count), dtype=torch.int32, device="cuda")
    norms = torch.empty((count, 2), dtype=torch.int64, device="cuda")

    def pack():
        ctx.ring_pack_device(words.data_ptr(), status[0].data_ptr(), x.data_ptr(), count, bits, mode, s)

    def unpack():
        ctx.ring_unpack_device(back.data_ptr(), status[1].data_ptr(), words.data_ptr(), count, bits, mode, s)

    def l2sq():
        ctx.ring_l2sq_device(x.data_ptr(), count, 1, norms.data_ptr(), s)

    # the torch route: what depends on the shape alone
    pos = torch.arange(total, dtype=torch.int64, device="cuda") * bits
    word, off = pos >> 6, pos & 63
    straddle = off + bits > 64
    word_hi = torch.where(straddle, word + 1, word)
    shift_hi = torch.where(straddle, 64 - off, torch.zeros_like(off))
    keep = torch.where(off == 0, torch.full_like(off, -1), (torch.ones_like(off) << (64 - off).clamp(max=63)) - 1)
    del pos
    mask, half = (1 << bits) - 1, (Q - 1) // 2
    t_words, t_back = torch.empty(count * wpe, dtype=torch.int64, device="cuda"), None

    def torch_pack():
        flat = x.reshape(-1)
        f = (torch.where(flat > half, flat - Q, flat) if mode == 0 else flat) & mask
        t_words.zero_()
        t_words.index_add_(0, word, f << off)
        t_words.index_add_(0, word_hi, torch.where(straddle, f >> shift_hi, torch.zeros_like(f)))

    def torch_unpack():
        nonlocal t_back
        f = (((t_words[word] >> off) & keep) | torch.where(straddle, t_words[word_hi] << shift_hi, torch.zeros_like(off))) & mask
        if mode == 0:
            v = f - ((f >> (bits - 1)) << bits)
            f = torch.where(v < 0, v + Q, v)
        t_back = f

    pack(), unpack(), torch_pack(), torch_unpack()
    torch.cuda.synchronize()
    row = {"shape": name, "n": n, "count": count, "bits": bits, "mode": "RESIDUE" if mode else "CENTRED", "input": kind, "q": Q,
           "input_bytes": total * 8, "packed_bytes": count * wpe * 8, "status_all_1": bool((status == 1).all()),
           "pack_equals_torch": bool(torch.equal(words.reshape(-1), t_words)), "unpack_equals_input": bool(torch.equal(back, x)),
           "torch_unpack_equals_input": bool(torch.equal(t_back.reshape(count, n), x))}
    row.update(timed([("pack", pack), ("torch_pack", torch_pack), ("unpack", unpack), ("torch_unpack", torch_unpack), ("l2sq", l2sq)], reps, warmup))
    moved = row["input_bytes"] + row["packed_bytes"]
    for which in ("pack", "unpack"):
        row[which + "_TB_per_s"] = round(moved / row[which]["us_median"] / 1e6, 3)
        other = row["torch_" + which]
        row["ratio_torch_%s_over_%s" % (which, which)] = round(other["us_median"] / row[which]["us_median"], 2)
        row["%s_below_torch_by_more_than_the_spreads" % which] = bool(other["us_median"] - row[which]["us_median"] > other["us_spread"] + row[which]["us_spread"])
        row["ratio_%s_over_l2sq" % which] = round(row[which]["us_median"] / row["l2sq"]["us_median"], 3)
    row["l2sq_TB_per_s"] = round(row["input_bytes"] / row["l2sq"]["us_median"] / 1e6, 3)
    row["bytes_moved_over_bytes_read"] = round(1 + bits / 64, 3)
    del word, off, straddle, word_hi, shift_hi, keep, t_words, t_back
    torch.cuda.empty_cache()
    # (d) the host forms on pinned buffers, wall clock
    lib = pkg._abi.lib()
    h_x, h_w, h_back = pkg.PinnedArray((count, n)), pkg.PinnedArray((count, wpe)), pkg.PinnedArray((count, n))
    h_status = np.zeros(count, dtype=np.int32)
    h_x.array[:] = x.cpu().numpy().view(np.uint64)
    # torch tensors over the same pinned pages, for the plain copies
    p_x, p_back = torch.from_numpy(h_x.array.view(np.int64)), torch.from_numpy(h_back.array.view(np.int64))

    def host_pack():
        assert lib.lsr_ntt_ring_pack_batch(ctx._h, h_w.ptr, h_status.ctypes.data, h_x.ptr, count, mode, bits) == 0

    def host_unpack():
        assert lib.lsr_ntt_ring_unpack_batch(ctx._h, h_back.ptr, h_status.ctypes.data, h_w.ptr, count, mode, bits) == 0

    def copy_down():
        p_back.copy_(x)

    def copy_up():
        back.copy_(p_x)

    # the route of a prover whose vector is already on the device, and of a verifier that wants it there: only packed words cross
    p_w = torch.from_numpy(h_w.array.view(np.int64))

    def device_pack_and_copy_down():
        pack()
        p_w.copy_(words)

    def copy_up_and_device_unpack():
        words.copy_(p_w)
        unpack()

    row["host"] = {"pack": wall(host_pack, host_reps), "unpack": wall(host_unpack, host_reps), "copy_unpacked_words_to_pinned_host": wall(copy_down, host_reps),
                   "copy_unpacked_words_from_pinned_host": wall(copy_up, host_reps),
                   "device_pack_then_copy_packed_words_to_pinned_host": wall(device_pack_and_copy_down, host_reps),
                   "copy_packed_words_from_pinned_host_then_device_unpack": wall(copy_up_and_device_unpack, host_reps)}
    row["host"]["device_route_equals_input"] = bool(torch.equal(back, x))
    row["host"]["ratio_copy_down_over_device_pack_and_copy"] = round(row["host"]["copy_unpacked_words_to_pinned_host"]["us_median"] /
                                                                     row["host"]["device_pack_then_copy_packed_words_to_pinned_host"]["us_median"], 2)
    row["host"]["ratio_copy_up_over_copy_and_device_unpack"] = round(row["host"]["copy_unpacked_words_from_pinned_host"]["us_median"] /
                                                                     row["host"]["copy_packed_words_from_pinned_host_then_device_unpack"]["us_median"], 2)
    row["host"]["host_pack_equals_device_pack"] = bool(np.array_equal(h_w.array.view(np.int64), words.cpu().numpy()))
    row["host"]["host_unpack_equals_input"] = bool(np.array_equal(h_back.array, h_x.array))
    row["host"]["ratio_copy_down_over_host_pack"] = round(row["host"]["copy_unpacked_words_to_pinned_host"]["us_median"] / row["host"]["pack"]["us_median"], 3)
    row["host"]["ratio_copy_up_over_host_unpack"] = round(row["host"]["copy_unpacked_words_from_pinned_host"]["us_median"] / row["host"]["unpack"]["us_median"], 3)
    row["host"]["words_per_packed_word"] = round(64 / bits, 2)
    row["host"]["torch_sees_the_buffers_as_pinned"] = bool(p_x.is_pinned())
    del p_x, p_back, p_w
    for h in (h_x, h_w, h_back):
        h.close()
    ctx.close()
    torch.cuda.empty_cache()
    return row


def main():
    reps, warmup, host_reps = int(os.environ.get("REPS", "12")), int(os.environ.get("WARMUP", "2")), int(os.environ.get("HOST_REPS", "5"))
    pkg = entry.load_package()
    rows = [measure(pkg, name, reps, warmup, host_reps) for name in os.environ.get("SHAPES", "ABCD")]
    out = {"tool": "ring_pack_bench", "reps": reps, "warmup": warmup, "host_reps": host_reps, "rows": rows,
           "all_equal": all(r["pack_equals_torch"] and r["unpack_equals_input"] and r["torch_unpack_equals_input"] and r["status_all_1"] and
                            r["host"]["host_pack_equals_device_pack"] and r["host"]["host_unpack_equals_input"] and r["host"]["device_route_equals_input"] for r in rows),
           "criterion_met_at_every_shape": all(r["pack_below_torch_by_more_than_the_spreads"] and r["unpack_below_torch_by_more_than_the_spreads"] for r in rows),
           "provenance": provenance.provenance()}
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
