"""The one piece of the reference that compiles on its own — cpp-core/src/utils.cpp's Gaussian sampler — checked against the
oracle's restatement of the same sampler.  Its output is recorded in tests/golden/reference_sampler.json
(tests/golden/make_reference_sampler.py, from the binary `make -C oracle ref` builds): per sigma the histogram of 400 000
draws, and its return code for every argument case.  The reference draws from std::random_device, so the comparison is
distributional: its histogram against the probabilities of the oracle's CDT table (the table itself is in an anonymous
namespace and cannot be read out)."""
import json
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_sampler.json")


@pytest.fixture(scope="module")
def ref():
    with open(GOLDEN) as f:
        return json.load(f)


def reference_samples(ref, sigma):
    """The recorded draws of the reference's sample_gaussian at sigma (order is irrelevant to every statistic below)."""
    h = ref["histograms"][repr(sigma)]
    samples = np.repeat(np.array(h["values"], dtype=np.int64), np.array(h["counts"], dtype=np.int64))
    assert samples.size == ref["draws"]
    return samples


def table_probabilities(cdf):
    """P(sample = +-k) from the 64-bit CDT: first k with cdf[k] >= u, u uniform on [0, 2^64); sign bit fair for k != 0."""
    edges = [int(x) for x in cdf]
    mass = [edges[0] + 1] + [edges[k] - edges[k - 1] for k in range(1, len(edges))]
    total = float(2**64)
    probs = {0: mass[0] / total}
    for k in range(1, len(mass)):
        probs[k] = probs[-k] = mass[k] / total / 2
    return probs


def chi_square(samples, probs, min_expected=20.0):
    n = len(samples)
    values, counts = np.unique(samples, return_counts=True)
    seen = dict(zip((int(v) for v in values), (int(c) for c in counts)))
    assert set(seen) <= set(probs), "a sample outside the table's support"
    stat, dof, tail_obs, tail_exp = 0.0, 0, 0, 0.0
    for v, p in probs.items():
        exp = p * n
        if exp < min_expected:
            tail_obs += seen.get(v, 0); tail_exp += exp
            continue
        stat += (seen.get(v, 0) - exp) ** 2 / exp
        dof += 1
    if tail_exp >= 1.0:
        stat += (tail_obs - tail_exp) ** 2 / tail_exp
        dof += 1
    return stat, dof - 1


@pytest.mark.parametrize("sigma", [3.19, 3.2, 1.0, 8.0])
def test_reference_sampler_follows_the_restated_table(ref, oracle, sigma):
    samples = reference_samples(ref, sigma)
    n = samples.size
    probs = table_probabilities(oracle.gaussian_cdf(sigma))
    assert abs(sum(probs.values()) - 1.0) < 1e-12
    bound = max(8, math.ceil(12.0 * sigma))
    assert int(np.abs(samples).max()) <= bound == max(probs)                 # utils.cpp:31-37 tail bound
    stat, dof = chi_square(samples, probs)
    # chi-square with `dof` degrees of freedom: mean dof, sd sqrt(2 dof); 6 sd is a < 1e-8 false-alarm rate
    assert stat < dof + 6.0 * math.sqrt(2.0 * dof), (sigma, stat, dof)
    assert abs(float(samples.mean())) < 6.0 * sigma / math.sqrt(n)           # test_utils.cpp:40-50 moments
    assert abs(float(samples.std()) - sigma) < 0.02 * sigma + 0.01


def test_restated_sampler_passes_the_same_check(oracle):
    """The oracle's own sampler (seeded ChaCha20 words through the same CDT scan) under the identical statistic."""
    for sigma in [3.19, 8.0]:
        samples = oracle.sample_gaussian_seeded(400_000, sigma, 0xC0FFEE, 16, 0)
        stat, dof = chi_square(samples, table_probabilities(oracle.gaussian_cdf(sigma)))
        assert stat < dof + 6.0 * math.sqrt(2.0 * dof)


def test_argument_contract_equals_the_reference(ref, oracle):
    buf = np.zeros(8, dtype=np.uint64)
    cases = [(None, 16, 3.2), (buf.ctypes.data, 0, 3.2), (buf.ctypes.data, 8, 0.0), (buf.ctypes.data, 8, -1.0), (buf.ctypes.data, 8, float("inf")),
             (buf.ctypes.data, 8, float("nan")), (buf.ctypes.data, 8, 3.19), (buf.ctypes.data, 1, 0.5)]
    recorded = ref["argument_contract"]
    assert len(recorded) == len(cases)
    for (ptr, length, sigma), rec in zip(cases, recorded):
        assert (rec["pointer"], rec["length"], rec["sigma"]) == (ptr is not None, length, repr(sigma))
        assert rec["rc"] == oracle.L.oracle_sample_gaussian(ptr, length, sigma), (length, sigma)


@pytest.mark.gpu
def test_gpu_sampler_against_the_reference_distribution(ref, pkg):
    """Two-sample check: the library's sample_gaussian (device ChaCha20 + CDT) against the reference's recorded output."""
    sigma = 3.19
    theirs = reference_samples(ref, sigma)
    n = theirs.size
    ours = pkg.sample_gaussian(n, sigma)
    lo, hi = int(min(theirs.min(), ours.min())), int(max(theirs.max(), ours.max()))
    a = np.bincount(theirs - lo, minlength=hi - lo + 1).astype(float)
    b = np.bincount(ours - lo, minlength=hi - lo + 1).astype(float)
    keep = (a + b) >= 40
    stat = float(((a[keep] - b[keep]) ** 2 / (a[keep] + b[keep])).sum())      # two-sample chi-square, equal sizes
    dof = int(keep.sum()) - 1
    assert stat < dof + 6.0 * math.sqrt(2.0 * dof), (stat, dof)
