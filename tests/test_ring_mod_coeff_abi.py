"""CPU suite: the coefficient context of a ring handle and the handle's twisted inner product (lsr_ring_mod_coeff_context,
lsr_ring_mod_dot_galois_batch, batch.h "ring products under any modulus") are declared, exported and mirrored in ctypes
and in RingMod; the refusals that read no handle come in batch.h's order on a machine without a GPU; and every exported function that
takes an NttContext is either SERVED on the coefficient context, REFUSED on it, or an ACCESSOR — the three lists below partition
them, so a context-taking entry point added later fails here until someone decides where it belongs.

The handle of the refusal tests is fake and never used as a handle: those refusals read nothing of it."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = [os.path.join(ROOT, "include", "lambda_snark", name) for name in ("batch.h", "ntt.h", "prover.h", "commitment.h", "r1cs.h", "utils.h", "types.h")]
BATCH_H = HEADERS[0]

NEW = {
    "lsr_ring_mod_coeff_context": ["h"],
    "lsr_ring_mod_dot_galois_batch": ["h", "c", "a", "b", "batch", "terms", "b_rows", "g"],
    "lsr_ring_mod_dot_galois_batch_device": ["h", "d_c", "d_a", "d_b", "batch", "terms", "b_rows", "g", "stream"],
}


def _both(*names):
    return [n + suffix for n in names for suffix in ("", "_device")]


# served on the coefficient context: the coefficient-wise calls, which read only q and n
SERVED = _both("lsr_ntt_ring_sample_batch", "lsr_ntt_ring_challenge_batch", "lsr_ntt_ring_opnorm_batch", "lsr_ntt_ring_pack_batch",
               "lsr_ntt_ring_unpack_batch", "lsr_ntt_ring_decompose_batch", "lsr_ntt_ring_recompose_batch", "lsr_ntt_ring_linf_batch",
               "lsr_ntt_ring_automorphism_batch", "lsr_ntt_ring_l2sq_batch", "lsr_ntt_ring_project_batch", "lsr_ntt_ring_project_matrix_batch",
               "lsr_ntt_ring_project_adjoint_batch", "lsr_ntt_ring_scalar_combine_batch") + [
    "lsr_ntt_ring_opnorm_prepare", "ntt_mul_pointwise", "ntt_mul_pointwise_batch", "lsr_ntt_mul_pointwise_device"]
# refused on it: everything that transforms.  The value is the lsr_ring_mod_* call the message names, or None where there is none
REFUSED = {
    "ntt_forward": None, "ntt_inverse": None, "ntt_forward_batch": None, "ntt_inverse_batch": None,
    "lsr_ntt_forward_batch_device": None, "lsr_ntt_inverse_batch_device": None,
    "lsr_ntt_forward_batch_sharded": None, "lsr_ntt_inverse_batch_sharded": None,
    "lsr_cyclic_ntt_forward_batch": None, "lsr_cyclic_ntt_inverse_batch": None,
    "lsr_ntt_ring_mul_batch": "lsr_ring_mod_mul_batch", "lsr_ntt_ring_mul_batch_device": "lsr_ring_mod_mul_batch_device",
    "lsr_ntt_ring_dot_batch": "lsr_ring_mod_dot_batch", "lsr_ntt_ring_dot_batch_device": "lsr_ring_mod_dot_batch_device",
    "lsr_ntt_ring_fold_batch": "lsr_ring_mod_fold_batch", "lsr_ntt_ring_fold_batch_device": "lsr_ring_mod_fold_batch_device",
    "lsr_ntt_ring_dot_galois_batch": "lsr_ring_mod_dot_galois_batch", "lsr_ntt_ring_dot_galois_batch_device": "lsr_ring_mod_dot_galois_batch_device",
    "lsr_ntt_ring_matrix_create": "lsr_ring_mod_matrix_create", "lsr_ntt_ring_matrix_create_device": "lsr_ring_mod_matrix_create_device",
    "lsr_ntt_ring_matrix_create_seeded": "lsr_ring_mod_matrix_create_seeded",
    "lsr_ntt_ring_gram_batch": "lsr_ring_mod_gram_batch", "lsr_ntt_ring_gram_batch_device": "lsr_ring_mod_gram_batch_device",
    "lsr_ntt_ring_gram_sym2_batch": "lsr_ring_mod_gram_sym2_batch", "lsr_ntt_ring_gram_sym2_batch_device": "lsr_ring_mod_gram_sym2_batch_device",
    "lsr_ntt_ring_gram_block": None,
    "lsr_ntt_ring_quadform_batch": None, "lsr_ntt_ring_quadform_batch_device": None,
}
# answer on it: the device, 0, the flavour, 8, 0; ntt_context_free does nothing
ACCESSORS = ["lsr_ntt_context_device", "lsr_ntt_context_root", "lsr_ntt_context_uses_f64", "lsr_ntt_handoff_bytes", "lsr_ntt_context_is_cyclic",
             "ntt_context_free"]


def _declarations(path):
    """{name: parameter text} of every function declared in one header (comments and preprocessor lines removed)"""
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r"^\s*#[^\n]*", "", text, flags=re.M)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(\w+)\s*\(([^;{}()]*)\)\s*(?:LSR_NOEXCEPT|noexcept)?\s*;", text)}


def context_taking_functions():
    names = []
    for path in HEADERS:
        names += [name for name, params in _declarations(path).items() if re.search(r"\bNttContext\b", params)]
    return names


def test_every_context_taking_function_is_served_refused_or_an_accessor():
    found = context_taking_functions()
    assert len(found) == len(set(found)) and len(found) >= 60, "the header scan lost its grip"
    lists = {"SERVED": set(SERVED), "REFUSED": set(REFUSED), "ACCESSORS": set(ACCESSORS)}
    assert len(SERVED) == len(lists["SERVED"]) and len(ACCESSORS) == len(lists["ACCESSORS"])
    for name in found:
        homes = [k for k, v in lists.items() if name in v]
        assert len(homes) == 1, (name, homes, "decide whether the coefficient context serves or refuses this entry point (DESIGN.md §5t)")
    listed = set().union(*lists.values())
    assert listed == set(found), ("listed but no longer declared with an NttContext", sorted(listed - set(found)))
    for name, instead in REFUSED.items():                      # a named replacement is a declared call on the handle
        if instead:
            assert instead in _declarations(BATCH_H), (name, instead)
    # the header keeps the same two lists
    raw = open(BATCH_H).read()
    section = raw[raw.index("The coefficient context (DESIGN.md section 5t)"):raw.index("typedef struct LsrRingMod LsrRingMod;")]
    served, refused = section[section.index("SERVED on it"):section.index("REFUSED on it")], section[section.index("REFUSED on it"):]
    for name, text in [(n, served) for n in SERVED] + [(n, refused) for n in REFUSED]:
        assert re.search(r"\b" + name + r"\b", text) or re.search(r"\b" + re.sub(r"_device$", "", name) + r"\b", text), name
    for word in ("coefficient context", "never free it", "NO twiddle tables", "first\n *   check after the context's own NULL check"):
        assert word in section, word


def test_batch_h_declares_the_new_functions_with_the_contract():
    declared = _declarations(BATCH_H)
    for name, want in NEW.items():
        assert name in declared, name
        assert [a.strip().split()[-1].lstrip("*") for a in declared[name].split(",")] == want, name
    raw = open(BATCH_H).read()
    section = raw[raw.index("The twisted inner product, n <= 4096"):raw.index("The coefficient context (DESIGN.md section 5t)")]
    for word in ("word for word", "g = 1 is lsr_ring_mod_dot_batch", "max_terms unchanged", "g even", "g >= 2n", "names the composed route",
                 "lsr_ntt_ring_dot_galois_batch_device on each prime context"):
        assert word in section, word
    composition = raw[raw.index("Composition.  Together with"):raw.index("The fused calls, n <= 4096:")]
    assert "coefficient context" in composition and "EVERY n" in composition


def test_library_exports_signatures_and_members(pkg):
    lib = pkg._abi.load_library()
    vp, size, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64
    assert pkg._abi.SIGNATURES["lsr_ring_mod_coeff_context"] == (vp, [vp])
    assert pkg._abi.SIGNATURES["lsr_ring_mod_dot_galois_batch"] == (ctypes.c_int, [vp, vp, vp, vp, size, size, size, u64])
    assert pkg._abi.SIGNATURES["lsr_ring_mod_dot_galois_batch_device"] == (ctypes.c_int, [vp, vp, vp, vp, size, size, size, u64, vp])
    for name in NEW:
        assert hasattr(lib, name), name
    for member in ("coeff_context", "ring_dot_galois", "ring_dot_galois_device"):
        assert hasattr(pkg.RingMod, member), member
    for name in list(SERVED) + list(REFUSED) + ACCESSORS:
        assert name in pkg._abi.SIGNATURES and hasattr(lib, name), name


def test_null_handle(pkg):
    lib = pkg._abi.load_library()
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.addressof(buf)
    assert lib.lsr_ring_mod_coeff_context(None) is None
    assert lib.lsr_ring_mod_dot_galois_batch(None, p, p, p, 1, 1, 1, 1) == -1
    assert pkg._abi.last_error().startswith("lsr_ring_mod_dot_galois_batch: NULL"), pkg._abi.last_error()
    assert lib.lsr_ring_mod_dot_galois_batch_device(None, p, p, p, 1, 1, 1, 1, None) == -1
    assert pkg._abi.last_error().startswith("lsr_ring_mod_dot_galois_batch_device: NULL"), pkg._abi.last_error()
    lib.ntt_context_free(None)                                  # still NULL-safe


@pytest.mark.parametrize("name", ["lsr_ring_mod_dot_galois_batch", "lsr_ring_mod_dot_galois_batch_device"])
def test_dot_galois_refusals_that_read_no_handle_in_the_documented_order(pkg, name):
    lib = pkg._abi.load_library()
    bufs = [(ctypes.c_uint64 * 64)() for _ in range(3)]
    h_buf = (ctypes.c_uint64 * 512)()                          # zeros: nothing of it is read here
    h, c, a, b = [ctypes.addressof(x) for x in [h_buf] + bufs]
    device = name.endswith("_device")

    def call(h, c, a, b, batch=2, terms=2, b_rows=2, g=3):
        return getattr(lib, name)(*([h, c, a, b, batch, terms, b_rows, g] + ([None] if device else [])))

    def refused(word, *args, **kw):
        assert call(*args, **kw) == -1
        msg = pkg._abi.last_error()
        assert msg.startswith(name + ":") and word in msg, msg

    good = (h, c, a, b)
    for i in range(4):                                         # (1) NULL handle or buffer, whatever the rest
        args = list(good)
        args[i] = None
        refused("NULL", *args, b_rows=3, terms=0, g=2)
    refused("b_rows must be 1 or batch", *good, b_rows=3, terms=0, g=2)          # (2) b_rows before (3) terms before (4) an even g
    refused("b_rows must be 1 or batch", *good, batch=0, b_rows=2)
    refused("terms must be at least 1", *good, terms=0, g=2)
    refused("terms must be at least 1", *good, terms=0, batch=0, b_rows=1)
    refused("is even", *good, g=2)
    refused("is even", *good, g=0, batch=0, b_rows=1)                             # (4) before (5) the empty call, a no-op
    assert call(*good, batch=0, b_rows=1, g=2**63 + 1) == 0                       # (g >= 2n is looked at by a non-empty call only)
    assert call(h, c, c, c, batch=0, b_rows=0) == 0
