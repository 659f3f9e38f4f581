"""GPU suite: the fused ring operations on cyclic contexts at the two-pass sizes n = 2^13 .. 2^17 — Goldilocks and both ordinary
primes (2^18 divides q - 1 for each, so every size exists).  Through mid_tile_log these sizes reach the MID instantiations LT = 9, 10,
11, 12 and 12 of the ring_mul, ring_dot and ring_fold tile kernels; ArithGold, which skips unit top twiddles and has its own carry
paths, reaches its MID instantiations nowhere else.  ring_matrix(m).matvec(x) is the composed route there, and ring_automorphism is
the gather kernel (STAGED = false).

Every word is compared exactly with a CPU reference: the oracle's cyclic_forward / cyclic_inverse around pointwise sums on Python
integers (ring_tile_model, ring_fold_model.fold_ref), and the scatter model automorphism_np.  No kernel result is compared with
another kernel's.  A negacyclic group (FP64 and the 60-bit prime) holds the gather kernel's sign path against the scatter model: the
group law and the ring homomorphism hold for sigma_{g^-1} as well as for sigma_g, the scatter model tells them apart.

Most of a case's time is the reference's: Python-integer products of up to 2^17 words per polynomial."""
import numpy as np
import pytest

import ring_tile_model as model
from ring_fold_model import fold_ref, vectors_needed
from ring_galois_model import automorphism_np, test_automorphism_np_equals_the_list_model  # noqa: F401 (collected here: CPU test)
from ring_tile_model import FLAVOURS
from test_ring_tile_sweep_gpu import _open

CYCLIC_FLAVOURS = ("gold", "cyc_f64", "cyc_u64")


@pytest.mark.gpu
@pytest.mark.parametrize("logn", range(13, 18))
@pytest.mark.parametrize("flavour", CYCLIC_FLAVOURS)
def test_cyclic_two_pass_operations(pkg, lib, oracle, flavour, logn):
    n = 1 << logn
    omega = model.omega_for(oracle, flavour, n)
    q, cyclic, ctx = _open(pkg, lib, flavour, n, omega)
    assert cyclic and FLAVOURS[flavour][1]
    rng = np.random.default_rng(300 * logn + len(flavour))
    ref = lambda fn, *args: fn(oracle, q, n, *args, cyclic, omega)      # noqa: E731
    lazy = model.goldilocks_lazy_carry(n) if flavour == "gold" else None
    where = (flavour, n)
    batch, terms = 2, 3

    # ring_mul: per-product b, one shared b
    a, b = model.planted(rng, q, batch, n), model.planted(rng, q, batch, n)
    if lazy is not None:
        a[1] = b[1] = lazy
    assert np.array_equal(ctx.ring_mul(a, b), ref(model.oracle_product, a, b)), (where, "ring_mul")
    assert np.array_equal(ctx.ring_mul(a, b[1]), ref(model.oracle_product, a, b[1])), (where, "ring_mul, shared b")

    # ring_dot: per-output b, one shared b
    a, b = model.planted(rng, q, batch * terms, n).reshape(batch, terms, n), model.planted(rng, q, batch * terms, n).reshape(batch, terms, n)
    if lazy is not None:
        a[1, 0] = b[1, 2] = b[0, 1] = lazy
    assert np.array_equal(ctx.ring_dot(a, b), ref(model.oracle_dot, a, b)), (where, "ring_dot")
    assert np.array_equal(ctx.ring_dot(a, b[1]), ref(model.oracle_dot, a, b[1])), (where, "ring_dot, shared b")

    # ring_fold: shared vectors, overlapping windows or disjoint vectors by size
    outputs, fold_terms, width = 2, 2, 2
    stride = (0, 1, fold_terms)[logn % 3]
    v = model.planted(rng, q, vectors_needed(outputs, fold_terms, stride) * width, n).reshape(-1, width, n)
    p = model.planted(rng, q, outputs * fold_terms, n).reshape(outputs, fold_terms, n)
    if lazy is not None:
        v[1, 1] = p[1, 0] = lazy
    assert np.array_equal(ctx.ring_fold(v, p, stride), fold_ref(oracle, q, n, v, p, stride, cyclic, omega)), (where, "ring_fold", stride)

    # ring_matrix(m).matvec(x): the composed route above n = 4096
    rows, cols = 2, 2
    m, x = model.planted(rng, q, rows * cols, n).reshape(rows, cols, n), model.planted(rng, q, batch * cols, n).reshape(batch, cols, n)
    if lazy is not None:
        m[0, 1] = x[1, 0] = lazy
    mat = ctx.ring_matrix(m)
    assert np.array_equal(mat.matvec(x), ref(model.oracle_matvec, m, x)), (where, "matvec")
    mat.close()

    # ring_automorphism: the gather kernel, N = n (no sign)
    x = model.planted(rng, q, batch, n)
    assert ctx.galois_conjugation == n - 1
    for g in (n - 1, n // 2 + 1, n - 5):
        assert np.array_equal(ctx.ring_automorphism(x, g), automorphism_np(x, g, q, 1)), (where, "ring_automorphism", g)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("logn", [13, 16, 17])
@pytest.mark.parametrize("flavour", ["f64", "u64_q60"])
def test_gather_automorphism_sign_path(pkg, lib, flavour, logn):
    """The gather kernel on negacyclic contexts (N = 2 n): the sign bit s & n of the source position, and g^-1 where g^-1 belongs.  At
    n >= 2^16 the product (n - 1) g^-1 passes 2^32 for one of the elements, so the masked 32-bit product is on the path."""
    n = 1 << logn
    q, cyclic, ctx = _open(pkg, lib, flavour, n, 0)
    assert not cyclic
    gs = (3, n + 1, 2 * n - 1, 2 * n - 5)
    assert n < 1 << 16 or any((n - 1) * pow(g, -1, 2 * n) >= 1 << 32 for g in gs)
    assert any(pow(g, -1, 2 * n) != g for g in gs)                    # an element that is not its own inverse: sigma_g is not sigma_{g^-1}
    x = model.planted(np.random.default_rng(logn + len(flavour)), q, 2, n)
    for g in gs:
        assert np.array_equal(ctx.ring_automorphism(x, g), automorphism_np(x, g, q, -1)), (flavour, n, g)
    ctx.close()
