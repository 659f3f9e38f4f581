"""What holds the one-chunk results of host_staging_cases.py to something other than the library: CHECKS[case](oracle, inputs, out)
compares the outputs `out` of a case, run under the default staging bound on the operands it left in host_staging_cases.INPUTS, with
the integer models of the calls (ring_gadget_model, ring_galois_model, ring_challenge_model, ring_mod_model, ring_mod_matvec_model,
ring_norm_model, ring_pack_model; the cyclic mat-vec: the CPU oracle's transforms around a pointwise product).  Only the test's own
process calls it: the child under the shrunk bound replays the case and nothing else.

Every word where the model is quick.  Where it is not (the Kronecker products of ring_mod_model at hundreds of outputs, the bit loops of
ring_pack_model) the model judges whole items: the first and the last item of every chunk the shrunk bound makes and every refused
item.  The calls that go in term groups (130 terms at n = 1024, 70 at n = 4096) are judged on three coefficients of every output, each
a full row of the negacyclic matrix over all terms.  The rest is pinned by the child's equality with these one-chunk results."""
import numpy as np

import ring_challenge_model as challenge_model
import ring_gadget_model as gadget_model
import ring_galois_model as galois_model
import ring_mod_matvec_model as mod_matvec_model
import ring_mod_model as mod_model
import ring_norm_model as norm_model
import ring_pack_model as pack_model
import ring_tile_model as tile_model
from host_staging_cases import GADGET_DIGITS, _wide


def edges(count, chunk, *more):
    """the first and the last item of every chunk of `chunk` items, and `more`"""
    return sorted({i for first in range(0, count, chunk) for i in (first, min(first + chunk, count) - 1)} | set(more))


def _same(got, want, what):
    want = np.asarray(want)
    assert got.dtype == want.dtype and np.array_equal(got, want), what


def gadget(oracle, inputs, out):
    for name, op in inputs.items():
        q, b = op["q"], op["b"]
        _same(out[name + " digits"], gadget_model.decompose(op["x"], q, b, GADGET_DIGITS), (name, "decompose"))
        _same(out[name + " recomposed"], gadget_model.recompose(op["z"], q, b), (name, "recompose"))
        _same(out[name + " linf"], gadget_model.linf(op["y"], q), (name, "linf"))


def matvec_gadget(oracle, inputs, out):
    for name, op in inputs.items():
        at = edges(70, 32)
        _same(out[name][at], mod_matvec_model.matvec_gadget(op["m"], op["x"][at], op["q"], op["b"], GADGET_DIGITS), name)


def matvec(oracle, inputs, out):
    for name, op in inputs.items():
        if name == "gold":
            _same(out[name], tile_model.oracle_matvec(oracle, op["q"], 1024, op["m"], op["x"], True, op["omega"]), name)
        else:
            at = edges(60, 25)
            _same(out[name][at], mod_matvec_model.matvec(op["m"], op["x"][at], op["q"]), name)


def automorphism(oracle, inputs, out):
    for name, op in inputs.items():
        for g in (5, 1023 if op["cyclic"] else 2047):
            _same(out[f"{name} g {g}"], galois_model.automorphism_np(op["x"], g, op["q"], 1 if op["cyclic"] else -1), (name, g))


def dot_galois(oracle, inputs, out):
    for name, op in inputs.items():
        for form, rows in ((" each", op["b"]), (" shared", op["b"][1])):
            _same(out[name + form], galois_model.galois_dot_ref(oracle, op["q"], 1024, op["a"], rows, op["g"], False, 0), (name, form))


def opnorm(oracle, inputs, out):
    for name, op in inputs.items():
        _same(out[name], _wide([challenge_model.opnorm(words, op["q"], op["cyclic"]) for words in op["x"].tolist()]), name)


def _mod_products(op, out, tag, at, positions=None):
    """dot and ring_dot_galois of a ring handle at the outputs `at`, with b per output and with the shared row b[1]: every word of them
    (ring_mod_model.negacyclic_dot), or with `positions` those coefficients (dot_coefficient, one row of the negacyclic matrix)"""
    q, a, b = op["q"], op["a"], op["b"]
    twisted = galois_model.automorphism_np(a[at], op["g"], q, -1)
    for form in (" each", " shared"):
        for call, lhs in (("dot", a[at]), ("galois", twisted)):
            for i, j in enumerate(at):
                terms_a, terms_b, got = lhs[i].tolist(), (b[j] if form == " each" else b[1]).tolist(), out[call + tag + form][j]
                if positions is None:
                    assert got.tolist() == mod_model.negacyclic_dot(terms_a, terms_b, q), (call, tag, form, j)
                else:
                    assert [int(got[k]) for k in positions] == [mod_model.dot_coefficient(terms_a, terms_b, q, k) for k in positions], (call, tag, form, j)


def ring_mod_mul_dot(oracle, inputs, out):
    op = inputs["mul"]
    at = edges(300, 128)
    for form in ("each", "shared"):
        want = [mod_model.negacyclic_mul(op["a"][j].tolist(), op["b"][j if form == "each" else 3].tolist(), op["q"]) for j in at]
        _same(out["mul " + form][at], np.array(want, dtype=np.uint64), ("mul", form))
    _mod_products(inputs["dot"], out, "", edges(100, 32))
    _mod_products(inputs["dot groups"], out, " groups", [0, 1, 2], positions=(0, 511, 1023))


def ring_mod_nested_groups(oracle, inputs, out):
    _mod_products(inputs["dot nested"], out, " nested", [0, 1], positions=(0, 2049, 4095))


def ring_mod_matvec(oracle, inputs, out):
    op, at = inputs["plain"], edges(60, 25)
    _same(out["plain"][at], mod_matvec_model.matvec(op["m"], op["x"][at], op["q"]), "plain")
    op, at = inputs["gadget"], edges(70, 32)
    _same(out["gadget"][at], mod_matvec_model.matvec_gadget(op["m"], op["x"][at], op["q"], op["b"], GADGET_DIGITS), "gadget")


def ring_mod_coeff(oracle, inputs, out):
    op = inputs["all"]
    q = op["q"]
    _same(out["l2sq"], _wide(norm_model.l2sq(q, op["v"])), "l2sq")
    at = edges(250, 110, 170, 240)
    words, status = pack_model.pack_array(op["x"][at], q, 10, pack_model.CENTRED)
    _same(out["words"][at], words, "pack")
    _same(out["status"][at], status, "pack status")
    back, status = pack_model.unpack_array(out["words"][at], 1024, q, 10, pack_model.CENTRED)
    _same(out["back"][at], back, "unpack")
    _same(out["back status"][at], status, "unpack status")
    at = edges(250, 84, 200)
    words, status = pack_model.pack_array(op["y"][at], q, 33, pack_model.RESIDUE)
    words[at.index(200), 0] |= np.uint64(1 << 32)         # (the case's invalid field)
    _same(out["residues"][at], words, "pack residue")
    _same(out["residue status"][at], status, "pack residue status")
    unpacked, status = pack_model.unpack_array(out["residues"][at], 1024, q, 33, pack_model.RESIDUE)
    _same(out["unpacked"][at], unpacked, "unpack residue")
    _same(out["unpacked status"][at], status, "unpack residue status")


CHECKS = {f.__name__: f for f in (gadget, matvec_gadget, matvec, automorphism, dot_galois, opnorm, ring_mod_mul_dot, ring_mod_nested_groups,
                                  ring_mod_matvec, ring_mod_coeff)}
