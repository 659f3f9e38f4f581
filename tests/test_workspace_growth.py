"""A refused workspace growth leaves no stale capacity behind (first finding): tests/c/workspace_growth_driver.cpp asks
DeviceBuffer::reserve and R1csScratch for 2^50 bytes, then checks that the call threw, that the owner is empty or untouched, that the
scratch's chunk did not advance and (with a device) that a following small request allocates again.  Without a device only the
refusals are checked.  The driver launches no kernel."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def run(cmd, **kw):
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, **kw)
    assert out.returncode == 0, out.stdout[-4000:]
    return out.stdout


def test_refused_growth_leaves_no_stale_capacity(pkg, tmp_path):
    import __graft_entry__ as entry
    exe = str(tmp_path / "workspace_growth")
    csrc = os.path.join(ROOT, "lambda-snark-r_amd/csrc")
    lib_dir = os.path.dirname(entry.LIB)
    run([HIPCC, "-std=c++17", "-O1", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
         "-x", "hip", os.path.join(ROOT, "tests/c/workspace_growth_driver.cpp"), "-x", "none",
         "-L" + lib_dir, "-llambda_snark_core", "-Wl,-rpath," + lib_dir, "-o", exe])
    assert "ok" in run([exe])
