"""GPU suite: the host-pointer forms of the ring calls past their first staging chunk (host_staged and host_staged_dot,
lsr_ring_call.hpp).  Each case of host_staging_cases.py runs here under the default bound, where its buffers are one
chunk, and in a fresh child under LAMBDA_SNARK_STAGING_MIB=1 (read once per process), where they are three or more: every output word,
status word and tries word must be equal.  The one-chunk results of the cases in host_staging_refs.CHECKS are first held to the integer
models of their calls, so that the two runs are not only compared with each other.

Call sites of the two loops in csrc/ and the case that takes each through three or more chunks:
    lsr_ring_sample.hip        sample                              sample, sample_small
    lsr_ring_challenge.hip     opnorm                              opnorm
                               challenge                           challenge
    lsr_ring_pack.hip          pack, unpack                        pack, pack_small, ring_mod_coeff
    lsr_ring_norm.hip          l2sq                                l2sq, ring_mod_coeff
                               project                             project
                               project_matrix                      project_matrix
                               project_adjoint                     project_adjoint
    lsr_ring_scalar.hip        scalar_combine                      scalar_combine, scalar_combine_term_groups
    lsr_ring_mul.hip           ring_mul                            ring_mul
    lsr_ring_dot.hip           ring_dot (host_staged_dot)          ring_dot
    lsr_ring_fold.hip          ring_fold                           ring_fold, ring_fold_term_groups
    lsr_ring_gram.hip          gram, gram_sym2                     ring_gram
    lsr_ring_quadform.hip      quadform                            ring_quadform
    lsr_ring_matvec.hip        matvec                              matvec
    lsr_ring_gadget.hip        decompose, recompose, linf          gadget
                               matvec_gadget                       matvec_gadget
    lsr_ring_galois.hip        automorphism                        automorphism
                               dot_galois (host_staged_dot)        dot_galois
    lsr_ring_mod.hip           mul, dot, dot_galois (..._dot)      ring_mod_mul_dot, ring_mod_nested_groups
    lsr_ring_mod_matvec.hip    matvec, matvec_gadget               ring_mod_matvec
                               matvec_bounded                      test_ring_mod_matvec_bounded_gpu.py
    lsr_ring_mod_gram.hip      gram, gram_sym2                     ring_mod_gram
    lsr_ring_mod_fold.hip      fold                                test_ring_mod_fold_gpu.py
    lsr_ring_mod_quadform.hip  quadform                            test_ring_mod_quadform_gpu.py"""
import os
import subprocess
import sys

import numpy as np
import pytest

import host_staging_cases as cases
import host_staging_refs as refs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as entry
import host_staging_cases as cases
np.savez(sys.argv[3], **cases.CASES[sys.argv[2]](entry.load_package()))
"""


def test_every_reference_belongs_to_a_case():
    assert set(refs.CHECKS) <= set(cases.CASES)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_chunked_staging_equals_one_chunk(pkg, oracle, tmp_path, name):
    assert "LAMBDA_SNARK_STAGING_MIB" not in os.environ, "the reference run takes the default bound"
    want = cases.CASES[name](pkg)
    if name in refs.CHECKS:
        refs.CHECKS[name](oracle, cases.INPUTS[name], want)
    script, out = tmp_path / "child.py", tmp_path / "out.npz"
    script.write_text(_CHILD)
    subprocess.run([sys.executable, str(script), ROOT, name, str(out)], check=True, env=dict(os.environ, LAMBDA_SNARK_STAGING_MIB="1"), timeout=300)
    got = np.load(str(out))
    assert sorted(got.files) == sorted(want)
    for key, value in want.items():
        assert got[key].dtype == value.dtype and np.array_equal(got[key], value), (name, key)
