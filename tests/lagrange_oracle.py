"""Test helper: an O(m^2) Python restatement of the reference's Lagrange (baseline) path (rust-api/lambda-snark/src/r1cs.rs:529-654,
746-828, 995-1065; lib.rs:747-980, 1016-1215) for any modulus, including the omega-domain rule of NTT_FRIENDLY_MODULUS and the
refusal where an interpolation denominator is not a unit.  tests/prover_replay.py restates the same path in O(m^3) on the
sequential domain only; tests/test_r1cs_lagrange_abi.py pins the two together.  Test infrastructure only — nothing here ships."""
import hashlib

import numpy as np

NTT_MODULUS = 18446744069414584321
QUIRK_MODULUS = 17592169062401           # NTT_FRIENDLY_MODULUS, r1cs.rs:529
ROOTS_OF_UNITY = {4: 981206394875, 8: 4268641988953, 16: 9400386778549, 32: 15690227524213, 64: 8332322609789, 128: 9249819209096,
                  256: 5221410271124, 512: 9594533594163, 1024: 11016271016603, 2048: 14373677444369, 4096: 11176258803537,
                  8192: 9037003627149}
FS_TAG = b"LAMBDA-SNARK-R-FS-v1"


class NotAUnit(ValueError):
    """mod_inverse of a non-unit: the reference panics (arith.rs:66-85, r1cs.rs:520-525)."""


def uses_ntt(m, q):
    """should_use_ntt (r1cs.rs:386-389) under the default fft-ntt feature"""
    return q == NTT_MODULUS and m >= 1 and (m & (m - 1)) == 0


def domain(m, q):
    """lagrange_basis (r1cs.rs:596-607): {omega^j} for the quirk modulus with m in ROOTS_OF_UNITY, else {0, ..., m-1}"""
    omega = ROOTS_OF_UNITY.get(m) if q == QUIRK_MODULUS else None
    if omega is None:
        return [j % q for j in range(m)]
    return [pow(omega, j, q) for j in range(m)]


def _linear_product(points, q):
    z = [1]
    for x in points:
        z = [((z[k - 1] if k else 0) - x * (z[k] if k < len(z) else 0)) % q for k in range(len(z) + 1)]
    return z


def vanishing_seq(m, q):
    """vanishing_poly(m, q, false): prod_{i<m} (X - i), m + 1 coefficients"""
    return _linear_product([i % q for i in range(m)], q)


def interpolation_rows(m, q):
    """[(w_i, P_i)] with P_i = Z / (X - x_i) and w_i = prod_{j != i} (x_i - x_j)^-1, so L[k][i] = w_i P_i[k]; NotAUnit otherwise"""
    xs = domain(m, q)
    z = _linear_product(xs, q)
    rows = []
    for i, x in enumerate(xs):
        p = [0] * m
        p[m - 1] = z[m]
        for k in range(m - 1, 0, -1):
            p[k - 1] = (z[k] + x * p[k]) % q
        d = 0
        for c in reversed(p):
            d = (d * x + c) % q
        try:
            w = pow(d, -1, q)
        except ValueError:
            raise NotAUnit(f"prod_(j != {i}) (x_i - x_j) = {d} is not a unit mod {q}") from None
        rows.append((w, np.array(p, dtype=object)))
    return rows


def interpolate_many(evals_list, q, rows=None):
    """lagrange_interpolate of several evaluation vectors of one length m (shared basis)"""
    m = len(evals_list[0])
    rows = rows or interpolation_rows(m, q)
    out = [np.zeros(m, dtype=object) for _ in evals_list]
    for i, (w, p) in enumerate(rows):
        for acc, ev in zip(out, evals_list):
            c = int(ev[i]) % q * w % q
            if c:
                acc += c * p
    return [[int(v) % q for v in acc] for acc in out]


def interpolate(evals, q):
    return interpolate_many([evals], q)[0]


def lagrange_basis_ntt(i, m, omega, q):
    """a literal restatement of r1cs.rs:610-654 (poly_mul_linear and the denominator product, then mod_inverse)"""
    poly = [1]
    powers = [1]
    for _ in range(1, m):
        powers.append(powers[-1] * omega % q)
    for j in range(m):
        if j == i:
            continue
        nxt = [0] * (len(poly) + 1)                 # poly_mul_linear(poly, omega^j): poly * (X - omega^j)
        for k, c in enumerate(poly):
            nxt[k + 1] = (nxt[k + 1] + c) % q
            nxt[k] = (nxt[k] - c * powers[j]) % q
        poly = nxt
    denom = 1
    for j in range(m):
        if j != i:
            denom = denom * ((powers[i] - powers[j]) % q) % q
    inv = pow(denom, -1, q)
    poly = [c * inv % q for c in poly]
    return poly + [0] * (m - len(poly))


def poly_mul(a, b, q):
    a = np.array([int(v) for v in a], dtype=object)
    out = np.zeros(len(a) + len(b) - 1, dtype=object)
    for j, y in enumerate(b):
        if int(y):
            out[j:j + len(a)] += int(y) * a
    return [int(v) % q for v in out]


def poly_div_vanishing(num, m, q):
    """poly_div_vanishing(num, m, q, false) (r1cs.rs:995-1065): the trimmed quotient, or None for a non-zero remainder"""
    zh = vanishing_seq(m, q)
    rem = np.array([int(v) % q for v in num], dtype=object)
    if len(rem) - 1 < m:
        return [0] if not any(int(v) for v in rem) else None
    zarr = np.array(zh, dtype=object)
    quot = [0] * (len(rem) - m)
    for i in range(len(quot) - 1, -1, -1):
        c = int(rem[i + m]) % q
        quot[i] = c
        if c:
            rem[i:i + m + 1] = (rem[i:i + m + 1] - c * zarr) % q
    if any(int(v) % q for v in rem):
        return None
    while len(quot) > 1 and quot[-1] == 0:
        quot.pop()
    return quot


def mat_vec(entries, m, z, q):
    """SparseMatrix::mul_vec (sparse_matrix.rs:259-289): values and witness words reduced mod q"""
    out = [0] * m
    for row, col, val in entries:
        out[row] = (out[row] + (int(val) % q) * (int(z[col]) % q)) % q
    return out


def quotient(evals, q, rows=None):
    """compute_quotient_poly on the baseline path from (A z, B z, C z): the trimmed Q, or None (unsatisfied / remainder)"""
    a, b, c = evals
    m = len(a)
    if any((x * y - w) % q for x, y, w in zip(a, b, c)):
        return None
    pa, pb, pc = interpolate_many([a, b, c], q, rows)
    ab = poly_mul(pa, pb, q)
    num = [(ab[k] - (pc[k] if k < m else 0)) % q for k in range(len(ab))]
    return poly_div_vanishing(num, m, q)


def eval_poly(poly, x, q):
    """r1cs.rs:362-373"""
    r = 0
    for c in reversed(poly):
        r = (r * x + int(c)) % q
    return r


def challenge_derive(public_inputs, words, q):
    """challenge.rs:102-134"""
    h = hashlib.sha3_256()
    h.update(FS_TAG)
    h.update(len(public_inputs).to_bytes(8, "little"))
    for v in public_inputs:
        h.update(int(v).to_bytes(8, "little"))
    h.update(len(words).to_bytes(8, "little"))
    h.update(np.asarray(words, dtype="<u8").tobytes())
    d = h.digest()
    return int.from_bytes(d[:8], "little") % q, d


def blind(quot, m, q, r):
    """poly_add(Q, r Z_H) with the dense sequential Z_H (lib.rs:877-910), trimmed"""
    zh = vanishing_seq(m, q)
    out = [((quot[k] if k < len(quot) else 0) + r * zh[k]) % q for k in range(max(len(quot), m + 1))]
    while len(out) > 1 and out[-1] == 0:
        out.pop()
    return out


def prove_one(entries, m, q, witness, n_public, commit, seed, r=None, rows=None):
    """prove_r1cs (r None) / prove_r1cs_zk for one witness: (row, 13 proof words, hash bytes, quotient length) or None.
    commit(message words mod q, seed) -> the commitment's words (it reduces mod its own modulus)."""
    evals = [mat_vec(e, m, witness, q) for e in entries]
    qq = quotient(evals, q, rows)
    if qq is None:
        return None
    qp = qq if r is None else blind(qq, m, q, r % q)
    row = np.asarray(commit(qp, seed), dtype=np.uint64)
    alpha, ha = challenge_derive([int(v) for v in witness[:n_public]], row, q)
    beta, hb = challenge_derive([alpha], row, q)
    pa, pb, pc = interpolate_many(evals, q, rows)
    ev = lambda p, x: eval_poly(p, x, q)
    qa, qb = ev(qp, alpha), ev(qp, beta)
    proof = [alpha, beta, qa, qb, ev(pa, alpha), ev(pb, alpha), ev(pc, alpha), ev(pa, beta), ev(pb, beta), ev(pc, beta), qa, qb,
             0 if r is None else r % q]
    return row, proof, ha + hb, len(qq)


# ---- verify_r1cs[_zk] with arith.rs's u64 / u128 semantics for any proof word ----
M64 = (1 << 64) - 1


def _sub_mod(a, b, q):
    d = (a + q - b) % (1 << 128)
    if d >= q:
        d = (d - q) % (1 << 128)
    return d & M64


def eval_vanishing(m, x, q):
    """r1cs.rs:424-442"""
    if uses_ntt(m, q):
        return _sub_mod(pow(x, m, q), 1, q)
    r = 1
    for i in range(m):
        r = r * _sub_mod(x, i % q, q) % q
    return r


def verify(proof, public, row, m, q, zk):
    alpha, _ = challenge_derive(public, row, q)
    if proof[0] != alpha:
        return 0
    beta, _ = challenge_derive([proof[0]], row, q)
    if proof[1] != beta:
        return 0
    for k in range(2):
        zh = eval_vanishing(m, proof[k], q)
        qv = proof[2 + k]
        if zk:
            qv = _sub_mod(qv, proof[12] * zh % q, q)
        if qv * zh % q != _sub_mod(proof[4 + 3 * k] * proof[5 + 3 * k] % q, proof[6 + 3 * k], q):
            return 0
    return int(proof[10] == proof[2] and proof[11] == proof[3])


# ---- circuits with exactly one satisfying extension of their free variables ----
def random_circuit(rng, m, free_vars, q, fan_in=2):
    """m constraints (A_i z)(B_i z) = z[free_vars + i]; A_i, B_i touch earlier variables only"""
    n = free_vars + m
    a, b, c = [], [], []
    for i in range(m):
        for mat in (a, b):
            for col in rng.choice(free_vars + i, size=min(fan_in, free_vars + i), replace=False):
                mat.append((i, int(col), int(rng.integers(0, 2**64, dtype=np.uint64))))     # values >= q exercise `val % modulus`
        c.append((i, free_vars + i, 1))
    return n, a, b, c


def extend_witness(free, m, a, b, q):
    z = [int(x) % q for x in free] + [0] * m
    rows_a, rows_b = [[] for _ in range(m)], [[] for _ in range(m)]
    for (i, col, v) in a:
        rows_a[i].append((col, v % q))
    for (i, col, v) in b:
        rows_b[i].append((col, v % q))
    f = len(free)
    for i in range(m):
        az = sum(v * z[col] for col, v in rows_a[i]) % q
        bz = sum(v * z[col] for col, v in rows_b[i]) % q
        z[f + i] = az * bz % q
    return np.array(z, dtype=np.uint64)
