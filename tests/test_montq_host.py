"""CPU test: the __host__ __device__ arithmetic of the Lagrange prove path (lsr_montq.hpp, lsr_lagrange_kernels.hpp) on the host,
against unsigned __int128, through the stand-alone driver tests/c/montq_host_driver.hip.  The driver is built as the library is built
(hipcc --offload-arch=gfx950), with UndefinedBehaviorSanitizer on the host pass, and run as a plain child process.  The device compile
of the same functions is what tests/test_lagrange_tiles_gpu.py runs."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def run(cmd, **kw):
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, **kw)
    assert out.returncode == 0, out.stdout[-4000:]
    return out.stdout


def test_montgomery_and_accumulator_arithmetic_on_the_host(tmp_path):
    exe = str(tmp_path / "montq_host")
    csrc = os.path.join(ROOT, "lambda-snark-r_amd/csrc")
    run([HIPCC, "-O1", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Wall", "-Wno-unused-function",
         "-Xarch_host", "-fsanitize=undefined", "-Xarch_host", "-fno-sanitize-recover=all",
         "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests/c/montq_host_driver.hip"), "-o", exe])
    out = run([exe], env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    assert out.startswith("ok: 15 moduli"), out[-2000:]
