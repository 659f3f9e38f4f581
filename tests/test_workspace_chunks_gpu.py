"""GPU suite: the batch loops of the n > 4096 device forms past their first workspace chunk — ring_mul_enqueue (lsr_ring_mul.hip,
DESIGN.md §5b) and matvec_composed (lsr_ring_matvec.hip, §5d).  Each case of workspace_chunk_cases.py runs here under the default
LAMBDA_SNARK_NTT_CHUNK_MIB, where a test-sized batch is one chunk, and in a fresh child under LAMBDA_SNARK_NTT_CHUNK_MIB=1 (read once per
process), where it is three: every output word must be equal.  The one-chunk results are first held, every word, to the CPU oracle's
composition forward, pointwise product, inverse (ring_tile_model.oracle_product / oracle_matvec), so that the two runs are not only
compared with each other."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ring_tile_model as tile_model
import workspace_chunk_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHUNK_BYTES = 1 << 20                           # LAMBDA_SNARK_NTT_CHUNK_MIB=1 (ntt_chunk_bytes, lsr_ntt.hip)


def ring_chunk_polys(n):                        # lsr_ring_mul.hip, ring_chunk_polys: half of the budget
    return max(1, (CHUNK_BYTES // 2) // (8 * n))


def matvec_chunk_polys(n):                      # lsr_ring_matvec.hip, matvec_chunk_polys: a third of the budget
    return max(1, (CHUNK_BYTES // 3) // (8 * n))


def ring_dot_chunk_polys(n):                    # lsr_ring_workspace.hpp, ring_dot_chunk_polys at n > 4096: a third of the budget
    return max(1, (CHUNK_BYTES // 3) // (8 * n))


def _split(count, chunk):
    return [min(chunk, count - first) for first in range(0, count, chunk)]


def test_the_shrunk_workspace_splits_the_cases_as_they_state():
    assert _split(cases.MUL_BATCH, ring_chunk_polys(cases.MUL_N)) == [8, 8, 3]
    assert _split(cases.FIVE_STAGE_BATCH, ring_chunk_polys(cases.FIVE_STAGE_N)) == [1, 1, 1]
    assert _split(cases.MATVEC_BATCH, matvec_chunk_polys(cases.MATVEC_N)) == [5, 5, 2]
    assert _split(cases.MATVEC_COLS, ring_dot_chunk_polys(cases.MATVEC_N)) == [5, 2]


def _same(got, want, what):
    assert got.dtype == want.dtype and np.array_equal(got, want), what


def _ring_mul_two_pass(oracle, inputs, out):
    for name, op in inputs.items():
        q, a, b, cyclic = op["q"], op["a"], op["b"], name == "gold"
        each = tile_model.oracle_product(oracle, q, cases.MUL_N, a, b, cyclic, op["omega"])
        shared = tile_model.oracle_product(oracle, q, cases.MUL_N, a, b[3], cyclic, op["omega"])
        for key in ("host each", "device apart", "device c is a", "device c is b"):
            _same(out[key], each, (name, key))
        for key in ("host shared", "device shared c is a"):
            _same(out[key], shared, (name, key))


def _ring_mul_five_stage(oracle, inputs, out):
    op = inputs["f64"]
    _same(out["each"], tile_model.oracle_product(oracle, op["q"], cases.FIVE_STAGE_N, op["a"], op["b"], False, 0), "each")
    _same(out["shared"], tile_model.oracle_product(oracle, op["q"], cases.FIVE_STAGE_N, op["a"], op["b"][1], False, 0), "shared")


def _matvec_composed(oracle, inputs, out):
    for name, op in inputs.items():
        want = tile_model.oracle_matvec(oracle, op["q"], cases.MATVEC_N, op["m"], op["x"], False, 0)
        _same(out[name + " host"], want, (name, "host"))
        _same(out[name + " device"], want, (name, "device"))


CHECKS = {"ring_mul_two_pass_f64": _ring_mul_two_pass, "ring_mul_two_pass_u64": _ring_mul_two_pass, "ring_mul_two_pass_gold": _ring_mul_two_pass,
          "ring_mul_five_stage": _ring_mul_five_stage, "matvec_composed": _matvec_composed}

_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as entry
import workspace_chunk_cases as cases
np.savez(sys.argv[3], **cases.CASES[sys.argv[2]](entry.load_package()))
"""


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cases.CASES))
def test_chunked_workspace_equals_one_chunk(pkg, oracle, tmp_path, name):
    assert "LAMBDA_SNARK_NTT_CHUNK_MIB" not in os.environ, "the reference run takes the default workspace"
    want = cases.CASES[name](pkg)
    CHECKS[name](oracle, cases.INPUTS[name], want)
    script, out = tmp_path / "child.py", tmp_path / "out.npz"
    script.write_text(_CHILD)
    subprocess.run([sys.executable, str(script), ROOT, name, str(out)], check=True, env=dict(os.environ, LAMBDA_SNARK_NTT_CHUNK_MIB="1"), timeout=300)
    got = np.load(str(out))
    assert sorted(got.files) == sorted(want)
    for key, value in want.items():
        assert got[key].dtype == value.dtype and np.array_equal(got[key], value), (name, key)
