"""The host-pointer calls of tests/test_host_staging_gpu.py, each on inputs it builds from a fixed seed: the test runs a case in its own
process under the default staging bound (one chunk) and in a fresh child under LAMBDA_SNARK_STAGING_MIB=1, and compares every array.

At 1 MiB the bound is 131072 words.  Each case states the chunk its call's formula gives there and is sized for at
least three chunks with a ragged last one; where a call has key or weight groups, `components` does not divide the chunk, so a group
straddles a chunk boundary; where it has a status, a refused item sits inside a later chunk, not at its start.

The cases from `gadget` on (and `matvec`) also leave their operands in INPUTS: the test's own process holds their one-chunk results to
the integer models (host_staging_refs.py); the child never reads it."""
import numpy as np

Q14 = 12289                    # n = 64 challenges
Q_NORTH = 17592169062401       # 44-bit NTT prime for n <= 4096 (FP64 kernels)
Q60 = 1152921504606584833      # 60-bit NTT prime (u64 Shoup kernels)
GOLD = 18446744069414584321    # CyclicNtt's modulus (Goldilocks kernels)
Q36 = (1 << 36) + 31           # RingMod: any modulus (odd, not NTT-friendly; n = 1024 carries it)
GADGET_BASE = {Q_NORTH: 12, Q60: 16, Q36: 10}      # base_log2 whose smallest admissible digit count under q is GADGET_DIGITS
GADGET_DIGITS = 4
UINT64_MAX = 2**64 - 1

INPUTS = {}                    # case name -> {key: operands} of the case's last run in this process


def _record(case, key, **operands):
    INPUTS.setdefault(case, {})[key] = operands


def _rand(rng, q, shape):
    return rng.integers(0, q, size=shape, dtype=np.uint64)


def _small(rng, q, shape, bound):
    """canonical words of centred coefficients in [-bound, bound]"""
    v = rng.integers(-bound, bound + 1, size=shape, dtype=np.int64)
    return np.where(v < 0, v + q, v).astype(np.uint64)


def _keys(rng, groups):
    return rng.integers(0, 1 << 63, size=(groups, 4), dtype=np.uint64)


def _wide(values):
    """Python ints below 2^128 as [..., 2] uint64 words"""
    flat = [int(v) for v in np.ravel(values)]
    return np.array([[v & (2**64 - 1), v >> 64] for v in flat], dtype=np.uint64)


def _contexts(pkg, n, flavours):
    """(name, context, q) for each flavour: "f64" (Q_NORTH), "u64" (Q60) on NTT-friendly primes, "gold" the cyclic Goldilocks ring"""
    for flavour in flavours:
        if flavour == "gold":
            yield flavour, pkg.CyclicNtt(n), GOLD
        else:
            q = Q_NORTH if flavour == "f64" else Q60
            ctx = pkg.NttContext(q, n, device=0)
            assert ctx.uses_f64 == (flavour == "f64")
            yield flavour, ctx, q


def sample(pkg):
    """n = 64: chunk 131072 / 64 = 2048 (2048 % 3 = 2), count 5000 = 2048 + 2048 + 904"""
    out, rng = {}, np.random.default_rng(1)
    keys = _keys(rng, 1667)
    for name, ctx, _ in _contexts(pkg, 64, ("f64", "gold")):
        out[name + " uniform"] = ctx.ring_sample(5000, pkg.RING_SAMPLE_UNIFORM, 0, keys, components=3, index_base=5)
        out[name + " ball"] = ctx.ring_sample(5000, pkg.RING_SAMPLE_BALL, 17, keys, components=3, index_base=5)
        ctx.close()
    return out


def sample_small(pkg):
    """n = 2 (the small kernel): chunk 131072 / 2 = 65536 (65536 % 7 = 2), count 140000 = 65536 + 65536 + 8928"""
    rng = np.random.default_rng(2)
    ctx = pkg.NttContext(Q14, 2, device=0)
    out = {"uniform": ctx.ring_sample(140000, pkg.RING_SAMPLE_UNIFORM, 0, _keys(rng, 20000), components=7),
           "bounded": ctx.ring_sample(140000, pkg.RING_SAMPLE_BOUNDED, 3, _keys(rng, 20000), components=7)}
    ctx.close()
    return out


def challenge(pkg):
    """n = 64: chunk 131072 / (64 + 1) = 2016 = 3 * 672, so components 5 (2016 % 5 = 1), count 4100 = 2016 + 2016 + 68.  T = 15 at
    weights (31, 10) rejects most first candidates: tries spread from 1 upwards."""
    out, rng = {}, np.random.default_rng(3)
    keys = _keys(rng, 820)
    for name, ctx in (("negacyclic", pkg.NttContext(Q14, 64, device=0)), ("cyclic", pkg.CyclicNtt(64))):
        c, tries = ctx.ring_challenge(4100, 31, 10, 15, keys, components=5, max_tries=64, index_base=2)
        assert len(set(tries[2016:].tolist())) > 2, "tries must vary past the first chunk"
        out[name], out[name + " tries"] = c, tries
        ctx.close()
    return out


def pack(pkg):
    """n = 4096, 10 bits: chunk 131072 / (4096 + 640) = 27, count 60 = 27 + 27 + 6; element 40 holds a coefficient of 600 > 511
    (status 0), element 58 a word >= q (status -1).  Unpack, RESIDUE at 44 bits: chunk 131072 / (2816 + 4096) = 18, count 60 =
    3 * 18 + 6; element 40 holds the field 2^44 - 1 >= q (status 0)."""
    rng = np.random.default_rng(4)
    ctx = pkg.NttContext(Q_NORTH, 4096, device=0)
    x = _small(rng, Q_NORTH, (60, 4096), 500)
    x[40, 7] = 600
    x[58, 9] = Q_NORTH
    words, status = ctx.ring_pack(x, 10)
    assert status.tolist() == [1] * 40 + [0] + [1] * 17 + [-1, 1]
    back, back_status = ctx.ring_unpack(words, 10)
    y = _rand(rng, Q_NORTH, (60, 4096))
    residues, residue_status = ctx.ring_pack(y, 44, pkg.RING_PACK_RESIDUE)
    residues[40, 0] |= np.uint64((1 << 44) - 1)
    unpacked, unpacked_status = ctx.ring_unpack(residues, 44, pkg.RING_PACK_RESIDUE)
    assert unpacked_status.tolist() == [1] * 40 + [0] + [1] * 19
    ctx.close()
    return {"words": words, "status": status, "back": back, "back status": back_status, "residues": residues, "residue status": residue_status,
            "unpacked": unpacked, "unpacked status": unpacked_status}


def pack_small(pkg):
    """n = 2 (the small kernels), 10 bits: chunk 131072 / (2 + 1) = 43690, count 90000 = 43690 + 43690 + 2620; elements 50001 (out
    of range) and 88000 (a word >= q) are refused; the packed word of element 60000 gets a padding bit for unpack to refuse"""
    rng = np.random.default_rng(5)
    ctx = pkg.NttContext(Q14, 2, device=0)
    x = _small(rng, Q14, (90000, 2), 500)
    x[50001, 1] = 700
    x[88000, 0] = Q14
    words, status = ctx.ring_pack(x, 10)
    assert status[50001] == 0 and status[88000] == -1 and int(status.sum()) == 89998 - 1
    words[60000, 0] |= np.uint64(1 << 40)
    back, back_status = ctx.ring_unpack(words, 10)
    assert back_status[60000] == 0 and back_status[43689] == 1
    ctx.close()
    return {"words": words, "status": status, "back": back, "back status": back_status}


def l2sq(pkg):
    """n = 1024, width 4: chunk 131072 / (4096 + 2) = 31, count 70 = 31 + 31 + 8"""
    out, rng = {}, np.random.default_rng(6)
    for name, ctx, q in _contexts(pkg, 1024, ("f64", "u64")):
        out[name] = _wide(ctx.ring_l2sq(_rand(rng, q, (70, 4, 1024))))
        ctx.close()
    return out


def project(pkg):
    """n = 1024, width 4: chunk 131072 / (4096 + 256) = 30 (30 % 4 = 2), count 70 = 30 + 30 + 10; vector 47 holds a coefficient
    above the bound (status 0), vector 65 a word >= q (status -1)"""
    rng = np.random.default_rng(7)
    ctx = pkg.NttContext(Q_NORTH, 1024, device=0)
    x = _small(rng, Q_NORTH, (70, 4, 1024), 5)
    x[47, 2, 100] = 6
    x[65, 0, 3] = Q_NORTH + 1
    p, status = ctx.ring_project(x, 5, _keys(rng, 18), components=4, index_base=9)
    assert status.tolist() == [1] * 47 + [0] + [1] * 17 + [-1] + [1] * 4
    ctx.close()
    return {"p": p, "status": status}


def project_matrix(pkg):
    """width n = 4096: chunk 131072 / 4096 = 32, rows 100 = 3 * 32 + 4 from row 5 on"""
    rng = np.random.default_rng(8)
    ctx = pkg.NttContext(Q_NORTH, 1024, device=0)
    out = {"rows": ctx.ring_project_matrix(_keys(rng, 1), 4, rows_first=5, rows=100, index_base=3)}
    ctx.close()
    return out


def project_adjoint(pkg):
    """sets 2, width n = 4096: chunk 131072 / 8192 = 16 (16 % 3 = 1), count 40 = 16 + 16 + 8; group 7 (vectors 21 .. 23) holds a
    weight >= q (status -1)"""
    out, rng = {}, np.random.default_rng(9)
    keys = _keys(rng, 14)
    for name, ctx, q in _contexts(pkg, 1024, ("f64", "gold")):
        weights = _rand(rng, q, (14, 2, 256))
        weights[7, 1, 200] = q
        for conjugate in (False, True):
            got, status = ctx.ring_project_adjoint(weights, 4, 40, keys, components=3, conjugate=conjugate, index_base=1)
            assert status.tolist() == [1] * 21 + [-1] * 3 + [1] * 16
            out[f"{name} conjugate {int(conjugate)}"], out[f"{name} conjugate {int(conjugate)} status"] = got, status
        ctx.close()
    return out


def scalar_combine(pkg):
    """width n = 4096, terms 3, sets 2, count 31: 32 vectors fit, so term_stride 1 takes chunks of (32 - 3 + 1) / (1 + 2) = 10 (31 =
    3 * 10 + 1) and term_stride 0 chunks of (32 - 3) / 2 = 14 (31 = 14 + 14 + 3); components 3 divides neither; group 5 (vectors
    15 .. 17) holds a weight >= q (status -1)"""
    out, rng = {}, np.random.default_rng(10)
    for name, ctx, q in _contexts(pkg, 1024, ("f64", "u64")):
        v, addend = _rand(rng, q, (33, 4, 1024)), _rand(rng, q, (31, 2, 4, 1024))
        weights = _rand(rng, q, (11, 2, 3))
        weights[5, 0, 2] = q + 2
        for ts in (1, 0):
            for add in (None, addend):
                got, status = ctx.ring_scalar_combine(v, weights, 31, term_stride=ts, components=3, addend=add)
                assert status.tolist() == [1] * 15 + [-1] * 3 + [1] * 13
                key = f"{name} stride {ts} addend {int(add is not None)}"
                out[key], out[key + " status"] = got, status
        ctx.close()
    return out


def scalar_combine_term_groups(pkg):
    """width n = 4096, terms 40, sets 2: 42 vectors do not fit the 32 of the bound — one output at a time, its terms in groups of
    32 - 2 = 30; group 1 (vectors 3 .. 5) holds a weight >= q"""
    out, rng = {}, np.random.default_rng(11)
    ctx = pkg.NttContext(Q_NORTH, 1024, device=0)
    v, addend = _rand(rng, Q_NORTH, (46, 4, 1024)), _rand(rng, Q_NORTH, (7, 2, 4, 1024))
    weights = _rand(rng, Q_NORTH, (3, 2, 40))
    weights[1, 1, 35] = Q_NORTH
    for add in (None, addend):
        got, status = ctx.ring_scalar_combine(v, weights, 7, term_stride=1, components=3, addend=add)
        assert status.tolist() == [1, 1, 1, -1, -1, -1, 1]
        out[f"addend {int(add is not None)}"], out[f"addend {int(add is not None)} status"] = got, status
    ctx.close()
    return out


def ring_mul(pkg):
    """n = 4096: each operand within the bound, chunk 131072 / 4096 = 32, batch 70 = 32 + 32 + 6"""
    out, rng = {}, np.random.default_rng(12)
    for name, ctx, q in _contexts(pkg, 4096, ("f64", "u64", "gold")):
        a, b = _rand(rng, q, (70, 4096)), _rand(rng, q, (70, 4096))
        out[name + " each"], out[name + " shared"] = ctx.ring_mul(a, b), ctx.ring_mul(a, b[3])
        ctx.close()
    return out


def ring_gram(pkg):
    """n = 1024, ra = rb = 2, width 2, batch 41.  Cross: chunk 131072 / (4096 + 4096 + 4096) = 10 (41 = 4 * 10 + 1); b is a: 131072 /
    (4096 + 4096) = 16 (16 + 16 + 9); symmetric: 131072 / (4096 + 3072) = 18 (18 + 18 + 5); sym2: 131072 / (4096 + 4096 + 3072) = 11
    (3 * 11 + 8)"""
    out, rng = {}, np.random.default_rng(13)
    for name, ctx, q in _contexts(pkg, 1024, ("f64", "u64")):
        a, b = _rand(rng, q, (41, 2, 2, 1024)), _rand(rng, q, (41, 2, 2, 1024))
        out[name + " cross"], out[name + " self"], out[name + " sym"] = ctx.ring_gram(a, b), ctx.ring_gram(a, a), ctx.ring_gram(a)
        out[name + " sym2"] = ctx.ring_gram_sym2(a, b)
        ctx.close()
    return out


def ring_quadform(pkg):
    """n = 1024, r = 3: chunk 131072 / (6144 + 3072 + 1024) = 12, batch 30 = 12 + 12 + 6"""
    out, rng = {}, np.random.default_rng(14)
    for name, ctx, q in _contexts(pkg, 1024, ("f64", "gold")):
        g, c = _rand(rng, q, (30, 6, 1024)), _rand(rng, q, (30, 3, 1024))
        out[name + " each"], out[name + " shared"] = ctx.ring_quadform(g, c), ctx.ring_quadform(g, c[1], offdiag=1)
        ctx.close()
    return out


def ring_mod_gram(pkg):
    """ring_gram's shapes and chunks on a RingMod handle with both bounds 128; family 27 holds a word above its bound (status 0: the
    third chunk of the cross form, the second of the others) and family 35 a word >= q (status -1)"""
    rng = np.random.default_rng(15)
    a, b = _small(rng, Q36, (41, 2, 2, 1024), 128), _small(rng, Q36, (41, 2, 2, 1024), 128)
    a[27, 1, 0, 5] = 129
    a[35, 0, 1, 6] = Q36
    want = [1] * 27 + [0] + [1] * 7 + [-1] + [1] * 5
    out = {}
    with pkg.RingMod(Q36, 1024, device=0) as ring:
        for name, (g, status) in (("cross", ring.gram(a, b, 128, 128)), ("self", ring.gram(a, a, 128, 128)), ("sym", ring.gram(a, None, 128)),
                                  ("sym2", ring.gram_sym2(a, b, 128, 128))):
            assert status.tolist() == want, name
            out[name], out[name + " status"] = g, status
    return out


def ring_fold(pkg):
    """n = 1024, width 2: 128 polynomials fit, so terms 3 at term_stride 1 take chunks of min(62, 128 / 3, 128 / 2) = 42, outputs 100 =
    42 + 42 + 16; the same at term_stride 0 (v goes up once)"""
    out, rng = {}, np.random.default_rng(16)
    for name, ctx, q in _contexts(pkg, 1024, ("f64", "gold")):
        v, p = _rand(rng, q, (102, 2, 1024)), _rand(rng, q, (100, 3, 1024))
        out[name + " stride 1"], out[name + " stride 0"] = ctx.ring_fold(v, p, term_stride=1), ctx.ring_fold(v, p, term_stride=0)
        ctx.close()
    return out


def ring_fold_term_groups(pkg):
    """n = 1024, width 2, terms 130 past 128 / 2: one output and one component at a time, its terms in groups of 128 + 2"""
    rng = np.random.default_rng(17)
    ctx = pkg.NttContext(Q_NORTH, 1024, device=0)
    v, p = _rand(rng, Q_NORTH, (132, 2, 1024)), _rand(rng, Q_NORTH, (3, 130, 1024))
    out = {"out": ctx.ring_fold(v, p, term_stride=1)}
    ctx.close()
    return out


def ring_dot(pkg):
    """n = 1024: 128 polynomials per operand; terms 4: chunk 32, batch 100 = 3 * 32 + 4; terms 130: one output at a time in groups of
    128 + 2 terms"""
    out, rng = {}, np.random.default_rng(18)
    for name, ctx, q in _contexts(pkg, 1024, ("f64", "u64")):
        a, b = _rand(rng, q, (100, 4, 1024)), _rand(rng, q, (100, 4, 1024))
        out[name + " each"], out[name + " shared"] = ctx.ring_dot(a, b), ctx.ring_dot(a, b[2])
        a, b = _rand(rng, q, (3, 130, 1024)), _rand(rng, q, (3, 130, 1024))
        out[name + " groups each"], out[name + " groups shared"] = ctx.ring_dot(a, b), ctx.ring_dot(a, b[1])
        ctx.close()
    return out


def matvec(pkg):
    """a 2 x 3 matrix at n = 1024: chunk 131072 / (3072 + 2048) = 25, batch 60 = 25 + 25 + 10"""
    out, rng = {}, np.random.default_rng(19)
    for name, ctx, q in _contexts(pkg, 1024, ("f64", "u64", "gold")):
        m, x = _rand(rng, q, (2, 3, 1024)), _rand(rng, q, (60, 3, 1024))
        mat = ctx.ring_matrix(m)
        out[name] = mat.matvec(x)
        _record("matvec", name, q=q, m=m, x=x, omega=ctx.omega if name == "gold" else 0)
        mat.close()
        ctx.close()
    return out


def _gadget_base(pkg, q):
    b = GADGET_BASE[q]
    assert pkg.ring_gadget_min_digits(q, b) == GADGET_DIGITS
    return b


def gadget(pkg):
    """n = 1024, 4 digits.  Decompose and recompose: chunk 131072 / (4096 + 1024) = 25, count 60 = 25 + 25 + 10.  linf: chunk 131072 /
    (1024 + 1) = 127, count 300 = 127 + 127 + 46; element 260 holds a word >= q (reported as 2^64 - 1)"""
    out, rng = {}, np.random.default_rng(20)
    for name, ctx, q in _contexts(pkg, 1024, ("f64", "u64")):
        b = _gadget_base(pkg, q)
        x, z, y = _rand(rng, q, (60, 1024)), _rand(rng, q, (60, GADGET_DIGITS, 1024)), _rand(rng, q, (300, 1024))
        y[260, 5] = q
        digits = ctx.ring_decompose(x, b, GADGET_DIGITS)
        assert np.array_equal(ctx.ring_recompose(digits, b), x)
        linf = ctx.ring_linf(y)
        assert np.flatnonzero(linf == np.uint64(UINT64_MAX)).tolist() == [260]
        out[name + " digits"], out[name + " recomposed"], out[name + " linf"] = digits, ctx.ring_recompose(z, b), linf
        _record("gadget", name, q=q, b=b, x=x, z=z, y=y)
        ctx.close()
    return out


def matvec_gadget(pkg):
    """a 2 x (2 * 4) matrix at n = 1024 against x of 2 columns: chunk 131072 / (2048 + 2048) = 32, batch 70 = 32 + 32 + 6"""
    out, rng = {}, np.random.default_rng(21)
    for name, ctx, q in _contexts(pkg, 1024, ("f64", "u64")):
        b = _gadget_base(pkg, q)
        m, x = _rand(rng, q, (2, 2 * GADGET_DIGITS, 1024)), _rand(rng, q, (70, 2, 1024))
        mat = ctx.ring_matrix(m)
        out[name] = mat.matvec_gadget(x, b, GADGET_DIGITS)
        _record("matvec_gadget", name, q=q, b=b, m=m, x=x)
        mat.close()
        ctx.close()
    return out


def automorphism(pkg):
    """n = 1024: chunk 131072 / (1024 + 1024) = 64, count 150 = 64 + 64 + 22; g = 5 and the conjugation g = N - 1 (N = 2 n; N = n on
    the cyclic ring)"""
    out, rng = {}, np.random.default_rng(22)
    for name, ctx, q in _contexts(pkg, 1024, ("f64", "gold")):
        assert ctx.galois_conjugation == (1023 if name == "gold" else 2047)
        x = _rand(rng, q, (150, 1024))
        for g in (5, ctx.galois_conjugation):
            out[f"{name} g {g}"] = ctx.ring_automorphism(x, g)
        _record("automorphism", name, q=q, x=x, cyclic=name == "gold")
        ctx.close()
    return out


def dot_galois(pkg):
    """n = 1024, g = 2 n - 1: 128 polynomials per operand; terms 4: chunk 32, batch 100 = 3 * 32 + 4; terms 130: one output at a time
    in groups of 128 + 2 terms, the sums waiting on the device in between; each with b per output and with one shared b row (which
    goes up with chunk 0 only while all its terms fit)"""
    out, rng = {}, np.random.default_rng(23)
    for name, ctx, q in _contexts(pkg, 1024, ("f64", "u64")):
        g = ctx.galois_conjugation
        for tag, batch, terms in (("", 100, 4), (" groups", 3, 130)):
            a, b = _rand(rng, q, (batch, terms, 1024)), _rand(rng, q, (batch, terms, 1024))
            twisted = ctx.ring_automorphism(a, g)
            for form, rows in ((" each", b), (" shared", b[1])):
                got = ctx.ring_dot_galois(a, rows, g)
                assert np.array_equal(got, ctx.ring_dot(twisted, rows)), (name, tag, form)
                out[name + tag + form] = got
            _record("dot_galois", name + tag, q=q, g=g, a=a, b=b)
        ctx.close()
    return out


def opnorm(pkg):
    """n = 64: chunk 131072 / (64 + 2) = 1985, count 4100 = 1985 + 1985 + 130.  The inputs are first candidates (T = 0) of ring_challenge
    at four weight pairs, interleaved, so that the norms vary inside every chunk."""
    out, rng = {}, np.random.default_rng(24)
    keys = _keys(rng, 4)
    for name, ctx in (("negacyclic", pkg.NttContext(Q14, 64, device=0)), ("cyclic", pkg.CyclicNtt(64))):
        parts = [ctx.ring_challenge(1025, k1, k2, 0, keys[i])[0] for i, (k1, k2) in enumerate(((31, 10), (16, 4), (8, 0), (40, 20)))]
        x = np.ascontiguousarray(np.stack(parts, axis=1).reshape(4100, 64))
        norms = ctx.ring_opnorm(x)
        assert len(set(norms[1985:].tolist())) > 2, "the norms must vary past the first chunk"
        out[name] = _wide(norms)
        _record("opnorm", name, q=GOLD if name == "cyclic" else Q14, x=x, cyclic=name == "cyclic")
        ctx.close()
    return out


def _ring_mod_products(ring, rng, q, n, case, shapes, g):
    """dot and ring_dot_galois of a RingMod at every (tag, batch, terms) of `shapes`, with b per output and with one shared b row"""
    out = {}
    for tag, batch, terms in shapes:
        a, b = _rand(rng, q, (batch, terms, n)), _rand(rng, q, (batch, terms, n))
        for form, rows in ((" each", b), (" shared", b[1])):
            out["dot" + tag + form], out["galois" + tag + form] = ring.dot(a, rows), ring.ring_dot_galois(a, rows, g)
        _record(case, "dot" + tag, q=q, g=g, a=a, b=b)
    return out


def ring_mod_mul_dot(pkg):
    """RingMod(Q36, 1024): 128 polynomials per staged operand.  mul: chunk 128, batch 300 = 128 + 128 + 44.  dot and ring_dot_galois
    (g = 2 n - 1): terms 4: chunk 32, batch 100 = 3 * 32 + 4; terms 130: one output at a time in staged groups of 128 + 2 terms, every
    group after the first accumulated into c (and the group of 128 split again at max_terms = 127 on the device)"""
    rng = np.random.default_rng(25)
    with pkg.RingMod(Q36, 1024, device=0) as ring:
        assert ring.max_terms == 127
        a, b = _rand(rng, Q36, (300, 1024)), _rand(rng, Q36, (300, 1024))
        out = {"mul each": ring.mul(a, b), "mul shared": ring.mul(a, b[3])}
        _record("ring_mod_mul_dot", "mul", q=Q36, a=a, b=b)
        out.update(_ring_mod_products(ring, rng, Q36, 1024, "ring_mod_mul_dot", (("", 100, 4), (" groups", 3, 130)), 2047))
    return out


def ring_mod_nested_groups(pkg):
    """RingMod(Q36, 4096), terms 70, batch 2: an operand holds 32 polynomials, so each output goes in staged groups of 32 + 32 + 6
    terms, and max_terms = 31 splits each group of 32 again into 31 + 1 inside ring_mod_dot_enqueue: the two groupings nest and the
    partial sums wait in c across both"""
    rng = np.random.default_rng(26)
    with pkg.RingMod(Q36, 4096, device=0) as ring:
        assert 2 <= ring.max_terms < 32 and 32 % ring.max_terms != 0
        return _ring_mod_products(ring, rng, Q36, 4096, "ring_mod_nested_groups", ((" nested", 2, 70),), 8191)


def ring_mod_matvec(pkg):
    """RingMod(Q36, 1024).  A 2 x 3 matrix: chunk 131072 / (3072 + 2048) = 25, batch 60 = 25 + 25 + 10.  The gadget product of a
    2 x (2 * 4) matrix with x of 2 columns: chunk 131072 / (2048 + 2048) = 32, batch 70 = 32 + 32 + 6"""
    out, rng = {}, np.random.default_rng(27)
    b = _gadget_base(pkg, Q36)
    with pkg.RingMod(Q36, 1024, device=0) as ring:
        m, x = _rand(rng, Q36, (2, 3, 1024)), _rand(rng, Q36, (60, 3, 1024))
        with ring.matrix(m) as mat:
            out["plain"] = mat.matvec(x)
        _record("ring_mod_matvec", "plain", q=Q36, m=m, x=x)
        m, x = _rand(rng, Q36, (2, 2 * GADGET_DIGITS, 1024)), _rand(rng, Q36, (70, 2, 1024))
        with ring.matrix(m) as mat:
            out["gadget"] = mat.matvec_gadget(x, b, GADGET_DIGITS)
        _record("ring_mod_matvec", "gadget", q=Q36, b=b, m=m, x=x)
    return out


def ring_mod_coeff(pkg):
    """the coefficient context of RingMod(2^32, 1024).  l2sq, width 4: chunk 131072 / (4096 + 2) = 31, count 70 = 31 + 31 + 8; vector
    47 holds a word >= q (2^128 - 1).  Pack, 10 bits: chunk 131072 / (1024 + 160) = 110, count 250 = 110 + 110 + 30; element 170 holds
    a coefficient of 600 > 511 (status 0), element 240 a word >= q (status -1).  Unpack, RESIDUE at 33 bits: chunk 131072 / (528 +
    1024) = 84, count 250 = 84 + 84 + 82; element 200 holds the field 2^32 >= q (status 0)."""
    q, rng = 1 << 32, np.random.default_rng(28)
    with pkg.RingMod(q, 1024, device=0) as ring:
        ctx = ring.coeff_context()
        v = _rand(rng, q, (70, 4, 1024))
        v[47, 2, 100] = q
        norms = ctx.ring_l2sq(v)
        assert [j for j, s in enumerate(norms.tolist()) if s == 2**128 - 1] == [47]
        x = _small(rng, q, (250, 1024), 500)
        x[170, 7] = 600
        x[240, 9] = q
        words, status = ctx.ring_pack(x, 10)
        assert status.tolist() == [1] * 170 + [0] + [1] * 69 + [-1] + [1] * 9
        back, back_status = ctx.ring_unpack(words, 10)
        y = _rand(rng, q, (250, 1024))
        residues, residue_status = ctx.ring_pack(y, 33, pkg.RING_PACK_RESIDUE)
        residues[200, 0] |= np.uint64(1 << 32)
        unpacked, unpacked_status = ctx.ring_unpack(residues, 33, pkg.RING_PACK_RESIDUE)
        assert unpacked_status.tolist() == [1] * 200 + [0] + [1] * 49
    _record("ring_mod_coeff", "all", q=q, v=v, x=x, y=y)
    return {"l2sq": _wide(norms), "words": words, "status": status, "back": back, "back status": back_status, "residues": residues,
            "residue status": residue_status, "unpacked": unpacked, "unpacked status": unpacked_status}


CASES = {f.__name__: f for f in (sample, sample_small, challenge, pack, pack_small, l2sq, project, project_matrix, project_adjoint, scalar_combine,
                                 scalar_combine_term_groups, ring_mul, ring_gram, ring_quadform, ring_mod_gram, ring_fold, ring_fold_term_groups,
                                 ring_dot, matvec, gadget, matvec_gadget, automorphism, dot_galois, opnorm, ring_mod_mul_dot,
                                 ring_mod_nested_groups, ring_mod_matvec, ring_mod_coeff)}
