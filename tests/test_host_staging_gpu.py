"""GPU suite: the host-pointer forms of the ring calls past their first staging chunk (host_staged, lsr_ring_call.hpp).
Each case of host_staging_cases.py runs here under the default bound, where its buffers are one chunk, and in a fresh child under
LAMBDA_SNARK_STAGING_MIB=1 (read once per process), where they are three or more: every output word, status word and tries word must
be equal."""
import os
import subprocess
import sys

import numpy as np
import pytest

import host_staging_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as entry
import host_staging_cases as cases
np.savez(sys.argv[3], **cases.CASES[sys.argv[2]](entry.load_package()))
"""


@pytest.mark.parametrize("name", list(cases.CASES))
def test_chunked_staging_equals_one_chunk(pkg, tmp_path, name):
    assert "LAMBDA_SNARK_STAGING_MIB" not in os.environ, "the reference run takes the default bound"
    want = cases.CASES[name](pkg)
    script, out = tmp_path / "child.py", tmp_path / "out.npz"
    script.write_text(_CHILD)
    subprocess.run([sys.executable, str(script), ROOT, name, str(out)], check=True, env=dict(os.environ, LAMBDA_SNARK_STAGING_MIB="1"), timeout=300)
    got = np.load(str(out))
    assert sorted(got.files) == sorted(want)
    for key, value in want.items():
        assert got[key].dtype == value.dtype and np.array_equal(got[key], value), (name, key)
