"""bench.py's command line: a plain run prints the headline line only (the secondary measurements and checks are behind
--full), and --dump-outputs writes what the last timed step computed, word for word the oracle's transform of the inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
Q16, N = 17592182243329, 65536


def test_bench_names_its_options():
    out = subprocess.run([sys.executable, BENCH, "--help"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0, out.stdout
    for opt in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs"):
        assert opt in out.stdout, opt


@pytest.mark.gpu
def test_plain_bench_run_dumps_the_last_step(tmp_path, oracle):
    dump = tmp_path / "outputs"
    polys, steps = 256, 3
    cmd = [sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--polys", str(polys), "--dump-outputs", str(dump)]
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stderr[-2000:]
    lines = [ln for ln in done.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, done.stdout[:2000]
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["unit"] == "NTT/s" and line["higher_is_better"] is True and line["dtype"] == "u64"
    assert abs(line["value"] - 2 * polys * steps / (line["ms_per_step"] * steps * 1e-3)) < 1e-6 * line["value"]
    assert not {"extra", "roofline", "cpu_baseline"} & set(line)             # those are --full's

    files = {p.name: p for p in dump.iterdir()}
    assert set(files) == {"ntt_forward.npy", "ntt_forward_inverse.npy", "sample_rows.npy"}
    assert sum(p.stat().st_size for p in files.values()) <= 64 * 2**20
    rows = np.load(files["sample_rows.npy"])
    fwd, after = np.load(files["ntt_forward.npy"]), np.load(files["ntt_forward_inverse.npy"])
    assert fwd.dtype == after.dtype == np.float64 and fwd.shape == after.shape == (len(rows), N)
    rows = rows.astype(np.int64)
    assert len(set(rows)) == len(rows) and rows.min() >= 0 and rows.max() < polys
    # polynomial i of the batch is splitmix64(0xDEADBEEF + i) mod q: a step (forward, then inverse) leaves it as it was
    inputs = np.stack([oracle.splitmix(0xDEADBEEF + int(i), Q16, N) for i in rows])
    assert np.array_equal(after.astype(np.uint64), inputs)
    pick = [0, len(rows) - 1]
    assert np.array_equal(fwd[pick].astype(np.uint64), oracle.ntt_forward(Q16, N, inputs[pick]))
