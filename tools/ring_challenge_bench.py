"""Operator-norm-bounded ring challenges on the device (lsr_ntt_ring_challenge_batch_device, lsr_ntt_ring_opnorm_batch_device; DESIGN.md
§5n), all legs of a group in one process, alternating after a warm-up; medians and spreads (max - min) of event-timed calls.  Prints
ONE JSON line and writes it to OUT.

  (a) kappa2 = 0, opnorm_bound = 0 against ring_sample_device BALL on the same keys, kappa = 41 at n = 64 and kappa = 60 at n = 4096,
      16384 elements: the outputs are identical (asserted) — the regression guard of the shuffle the two kernels share.
  (b) the rejecting sampler (kappa2 = 0, the only shape the composed route can draw) at n = 64 and n = 1024, 16384 elements, against
      the route without it: ring_sample_device BALL for every pending element (a fresh stream index per round), torch.fft of the
      twisted candidates, a masked keep, repeat until none is pending.  T is chosen so that the model's acceptance rate over 400
      candidates lies between 0.1 and 0.4 (recorded).
  (c) LaBRADOR's shape (31, 10, T = 15, n = 64) at 16 x 1024 elements, max_tries = 256: challenges per second and the tries.
  (d) the stand-alone norm at n = 64 (16384 elements) and n = 4096 (256 elements) of random coefficients up to 2^15 against torch.fft
      of the twisted coefficients in complex128 with a max over the points.
env REPS (default 20), WARMUP (2), OUT (default profiles/r30_ring_challenge_bench.json)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import __graft_entry__ as entry  # noqa: E402
import oracle_binding  # noqa: E402
import provenance  # noqa: E402
import ring_challenge_model as model  # noqa: E402
from ring_sample_model import key_from_seed  # noqa: E402

Q = 17592169062401
COUNT = 16384
MODEL_SAMPLES = 400


def stats(times_us):
    return {"us_median": round(float(np.median(times_us)), 1), "us_min": round(float(np.min(times_us)), 1), "us_max": round(float(np.max(times_us)), 1),
            "us_spread": round(float(np.max(times_us) - np.min(times_us)), 1)}


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
    return {k: stats(t) for k, t in times.items()}


def device_key(pkg, seed):
    return torch.from_numpy(pkg.ring_sample_key(seed).view(np.int64)).cuda()


def twist(n):
    return torch.exp(1j * torch.pi * torch.arange(n, device="cuda", dtype=torch.float64) / n)


def float_norms(x, q, tw):
    """the largest |c(zeta)| of every row of canonical words, by an FFT of the twisted centred coefficients"""
    centred = torch.where(x > q // 2, x - q, x).to(torch.float64)
    return torch.fft.fft(centred * tw, dim=-1).abs().amax(dim=-1)


def leg_a(pkg, n, kappa, reps, warmup):
    ctx = pkg.NttContext(Q, n, device=0)
    s = torch.cuda.current_stream().cuda_stream
    key = device_key(pkg, 1)
    ball, mine = (torch.empty((COUNT, n), dtype=torch.int64, device="cuda") for _ in range(2))
    tries = torch.empty(COUNT, dtype=torch.int32, device="cuda")
    legs = (("ring_sample_ball", lambda: ctx.ring_sample_device(ball.data_ptr(), COUNT, pkg.RING_SAMPLE_BALL, kappa, key.data_ptr(), COUNT, stream=s)),
            ("ring_challenge_no_bound", lambda: ctx.ring_challenge_device(mine.data_ptr(), tries.data_ptr(), COUNT, kappa, 0, 0, key.data_ptr(), COUNT,
                                                                           max_tries=1, stream=s)))
    rows = alternate(legs, reps, warmup)
    assert torch.equal(ball, mine) and bool((tries == 1).all())
    ctx.close()
    rows.update(n=n, kappa=kappa, count=COUNT, outputs_identical=True,
                challenge_over_ball=round(rows["ring_challenge_no_bound"]["us_median"] / rows["ring_sample_ball"]["us_median"], 3))
    return rows


def leg_b(pkg, oracle, n, kappa, bound, reps, warmup):
    _, tries, _ = model.challenge(oracle, Q, n, MODEL_SAMPLES, kappa, 0, bound, 1, [key_from_seed(1)], MODEL_SAMPLES)
    rate = float((tries == 1).mean())
    assert 0.1 <= rate <= 0.4, rate
    ctx = pkg.NttContext(Q, n, device=0)
    ctx.ring_opnorm_prepare()
    s = torch.cuda.current_stream().cuda_stream
    key = device_key(pkg, 1)
    mine, composed, cand = (torch.empty((COUNT, n), dtype=torch.int64, device="cuda") for _ in range(3))
    d_tries = torch.empty(COUNT, dtype=torch.int32, device="cuda")
    tw = twist(n)
    rounds = []

    def composed_route():
        pending = torch.arange(COUNT, device="cuda")
        done = 0
        while pending.numel():
            p = pending.numel()
            # every pending element under a fresh stream index: round r draws indices r COUNT ..
            ctx.ring_sample_device(cand.data_ptr(), p, pkg.RING_SAMPLE_BALL, kappa, key.data_ptr(), p, index_base=done * COUNT, stream=s)
            keep = float_norms(cand[:p], Q, tw) <= bound
            composed[pending[keep]] = cand[:p][keep]
            pending = pending[~keep]                         # (its size is read on the host: one synchronisation per round)
            done += 1
        rounds.append(done)
    legs = (("ring_challenge", lambda: ctx.ring_challenge_device(mine.data_ptr(), d_tries.data_ptr(), COUNT, kappa, 0, bound, key.data_ptr(), COUNT,
                                                                  max_tries=256, stream=s)),
            ("composed_ball_fft_keep", composed_route))
    rows = alternate(legs, reps, warmup)
    got = d_tries.cpu().numpy()
    assert (got >= 1).all() and bool((float_norms(mine, Q, tw) <= bound + 1e-6).all())
    ctx.close()
    rows.update(n=n, kappa=kappa, opnorm_bound=bound, count=COUNT, model_acceptance_rate=round(rate, 4), model_samples=MODEL_SAMPLES,
                mean_tries=round(float(got.mean()), 3), max_tries_seen=int(got.max()), composed_rounds=int(np.median(rounds)),
                composed_over_challenge=round(rows["composed_ball_fft_keep"]["us_median"] / rows["ring_challenge"]["us_median"], 2))
    return rows


def leg_c(pkg, reps, warmup):
    n, groups, components = 64, 16, 1024
    ctx = pkg.NttContext(Q, n, device=0)
    ctx.ring_opnorm_prepare()
    s = torch.cuda.current_stream().cuda_stream
    keys = torch.from_numpy(np.stack([pkg.ring_sample_key(100 + g) for g in range(groups)]).view(np.int64)).cuda()
    count = groups * components
    out, tries = torch.empty((count, n), dtype=torch.int64, device="cuda"), torch.empty(count, dtype=torch.int32, device="cuda")
    rows = alternate((("ring_challenge", lambda: ctx.ring_challenge_device(out.data_ptr(), tries.data_ptr(), count, 31, 10, 15, keys.data_ptr(),
                                                                          components, max_tries=256, stream=s)),), reps, warmup)
    got = tries.cpu().numpy()
    assert (got >= 1).all()
    ctx.close()
    rows.update(n=n, kappa1=31, kappa2=10, opnorm_bound=15, count=count, mean_tries=round(float(got.mean()), 3), max_tries_seen=int(got.max()),
                m_challenges_per_s=round(count / rows["ring_challenge"]["us_median"], 3),
                m_candidates_per_s=round(float(got.sum()) / rows["ring_challenge"]["us_median"], 3))
    return rows


def leg_d(pkg, n, count, reps, warmup):
    ctx = pkg.NttContext(Q, n, device=0)
    ctx.ring_opnorm_prepare()
    s = torch.cuda.current_stream().cuda_stream
    top = model.MAX_COEFFICIENT
    c = np.random.default_rng(n).integers(-top, top + 1, size=(count, n))
    x = torch.from_numpy(np.where(c < 0, c + Q, c).astype(np.int64)).cuda()
    out = torch.empty((count, 2), dtype=torch.int64, device="cuda")
    tw = twist(n)
    ref = []
    legs = (("ring_opnorm", lambda: ctx.ring_opnorm_device(x.data_ptr(), count, out.data_ptr(), stream=s)),
            ("torch_fft_abs_max", lambda: ref.append(float_norms(x, Q, tw))))
    rows = alternate(legs, reps, warmup)
    words = out.cpu().numpy().view(np.uint64)
    mine = np.array([((int(lo) | (int(hi) << 64)) ** 0.5) / model.SCALE for lo, hi in words.tolist()])
    worst = float(np.abs(mine - ref[-1].cpu().numpy()).max())
    assert worst <= n * top / 2**30.5 + 1e-6, worst
    ctx.close()
    rows.update(n=n, count=count, largest_difference_from_the_float_norm=worst,
                fft_over_opnorm=round(rows["torch_fft_abs_max"]["us_median"] / rows["ring_opnorm"]["us_median"], 2))
    return rows


def main():
    reps, warmup = int(os.environ.get("REPS", "20")), int(os.environ.get("WARMUP", "2"))
    path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "r30_ring_challenge_bench.json"))
    pkg, oracle = entry.load_package(), oracle_binding.load()
    out = {"tool": "ring_challenge_bench", "reps": reps, "warmup": warmup, "q": Q,
           "a_no_bound_against_ball": [leg_a(pkg, 64, 41, reps, warmup), leg_a(pkg, 4096, 60, reps, warmup)],
           "b_rejecting_against_composed": [leg_b(pkg, oracle, 64, 41, 12, reps, warmup), leg_b(pkg, oracle, 1024, 41, 15, reps, warmup)],
           "c_labrador": leg_c(pkg, reps, warmup),
           "d_norm_against_fft": [leg_d(pkg, 64, COUNT, reps, warmup), leg_d(pkg, 4096, 256, reps, warmup)],
           "provenance": provenance.provenance()}
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
