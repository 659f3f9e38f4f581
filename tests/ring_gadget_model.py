"""Reference model of the gadget decomposition (batch.h "gadget decomposition") in Python integers: admissibility and the
minimum digit count, the balanced carry-free digits, G^-1 of a vector, the gadget product back, the centred l-infinity norm and a
schoolbook ring product for the smallest fused-product cases."""
import numpy as np

Q44 = 17592180539393             # 44-bit prime, 2^18 | q - 1: every n up to 2^17 (FP64 kernels)
Q_NORTH = 17592169062401         # the benchmark's prime (n <= 4096)
Q60 = 1152921504606584833
Q14 = 12289
GOLDILOCKS = 18446744069414584321
MODULI = (Q_NORTH, Q44, Q60, Q14, GOLDILOCKS)
UINT64_MAX = 2**64 - 1

# the tables of the issue: q -> {b: minimum digits}
MIN_DIGITS_TABLE = {
    Q_NORTH: {2: 23, 3: 15, 4: 12, 8: 6, 11: 5, 12: 4, 15: 3, 16: 3, 22: 2, 23: 2, 32: 2},
    Q44: {2: 23, 3: 15, 4: 12, 8: 6, 11: 5, 12: 4, 15: 3, 16: 3, 22: 2, 23: 2, 32: 2},
    Q60: {2: 31, 3: 21, 4: 16, 8: 8, 11: 0, 16: 4, 32: 2},
    Q14: {2: 8, 3: 5, 4: 4, 8: 2, 11: 2, 12: 2, 16: 0},
}


def offset(b, digits):
    """B/2 in every one of the `digits` positions."""
    base = 1 << b
    return (base // 2) * ((base**digits - 1) // (base - 1))


def admissible(q, b, digits):
    if not (2 <= b <= 32 and digits >= 1 and b * digits <= 64):
        return False
    base, off = 1 << b, offset(b, digits)
    return base // 2 <= q // 2 and (q - 1) // 2 <= off and q // 2 <= base**digits - 1 - off


def min_digits(q, b):
    if not 2 <= b <= 32:
        return 0
    return next((d for d in range(1, 64 // b + 1) if admissible(q, b, d)), 0)


def centred(x, q):
    return x if x <= q // 2 else x - q


def digits_of(x, q, b, digits):
    """The signed digits z_0 .. z_{D-1} of the canonical word x."""
    u = centred(x, q) + offset(b, digits)
    assert 0 <= u < (1 << (b * digits))
    return [((u >> (b * d)) & ((1 << b) - 1)) - (1 << (b - 1)) for d in range(digits)]


def decompose(x, q, b, digits):
    """x: uint64 array [..., n] -> [..., digits, n] canonical digit residues."""
    x = np.asarray(x, dtype=np.uint64)
    flat = [digits_of(int(w), q, b, digits) for w in x.reshape(-1)]
    z = np.array([[zd % q for zd in zs] for zs in flat], dtype=np.uint64).reshape(x.shape + (digits,))
    return np.ascontiguousarray(np.moveaxis(z, -1, -2))


def gadget_inverse(x, q, b, digits):
    """x: [batch, xcols, n] -> [batch, xcols * digits, n], column c * digits + d = digit d of x[., c]."""
    z = decompose(x, q, b, digits)                      # [batch, xcols, digits, n]
    return z.reshape(x.shape[0], x.shape[1] * digits, x.shape[2])


def recompose(z, q, b):
    """z: [..., digits, n] canonical residues (short or not) -> [..., n]."""
    z = np.asarray(z, dtype=np.uint64)
    digits = z.shape[-2]
    acc = np.zeros(z.shape[:-2] + z.shape[-1:], dtype=object)
    for d in range(digits):
        acc = (acc + z[..., d, :].astype(object) * pow(1 << b, d, q)) % q
    return acc.astype(np.uint64)


def linf(x, q):
    """x: [..., n] -> [...] max |centred|, UINT64_MAX where a word is >= q."""
    x = np.asarray(x, dtype=np.uint64)
    out = []
    for elem in x.reshape(-1, x.shape[-1]):
        words = [int(w) for w in elem]
        out.append(UINT64_MAX if any(w >= q for w in words) else max(abs(centred(w, q)) for w in words))
    return np.array(out, dtype=np.uint64).reshape(x.shape[:-1])


def ring_mul_schoolbook(a, b, q, cyclic=False):
    n = len(a)
    out = [0] * n
    for i in range(n):
        for j in range(n):
            k, term = i + j, int(a[i]) * int(b[j])
            if k >= n:
                k -= n
                term = term if cyclic else -term
            out[k] = (out[k] + term) % q
    return out


def matvec_schoolbook(m, x, q, cyclic=False):
    """m: [rows, cols, n], x: [batch, cols, n] -> [batch, rows, n] by the definition."""
    rows, cols, n = m.shape
    y = np.zeros((x.shape[0], rows, n), dtype=np.uint64)
    for j in range(x.shape[0]):
        for r in range(rows):
            acc = [0] * n
            for c in range(cols):
                acc = [(s + t) % q for s, t in zip(acc, ring_mul_schoolbook(m[r, c], x[j, c], q, cyclic))]
            y[j, r] = np.array(acc, dtype=np.uint64)
    return y
