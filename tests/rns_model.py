"""Pure-Python model of the two-prime RNS commitment definition: moduli rule, message term, CRT lift, rounded decode,
row layout.  The GPU tests compare the library with it; nothing here touches the library."""

RNS_MAGIC = int.from_bytes(b"LSRR0001", "little")
RNS_HEADER_WORDS = 6


def is_prime(n):
    """Deterministic Miller-Rabin below 2^64 (the first twelve primes as witnesses)."""
    if n < 2:
        return False
    witnesses = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    for p in witnesses:
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d //= 2
        s += 1
    for a in witnesses:
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def largest_prime_1mod(factor, bits, skip=()):
    cand = ((2**bits - 1) // factor) * factor + 1
    while cand > 2 ** (bits - 1):
        if cand not in skip and is_prime(cand):
            return cand
        cand -= factor
    return 0


def rns_moduli(n):
    """q1: the default context's modulus for this n; q2: the largest 44-bit prime = 1 (mod 2n) other than q1."""
    q1 = 17592169062401 if n <= 4096 else largest_prime_1mod(2 * n, 44)
    return q1, largest_prime_1mod(2 * n, 44, skip=(q1,))


def plain_modulus(n):
    return largest_prime_1mod(2 * n, 20)


def round_div(a, b):
    """round(a / b) for non-negative a, odd b (no ties)."""
    return (2 * a + b) // (2 * b)


def message_term(m, t, q1, q2, qi):
    """round(Q (m mod t) / t) mod q_i"""
    return round_div(q1 * q2 * (m % t), t) % qi


def single_prime_term(m, t, qi):
    """round(q_i (m mod t) / t): what a single-prime commitment under q_i embeds"""
    return round_div(qi * (m % t), t)


def crt_lift(x1, x2, q1, q2):
    return x1 + q1 * (((x2 - x1) * pow(q1, -1, q2)) % q2)


def decode(x1, x2, t, q1, q2):
    big = q1 * q2
    return ((t * crt_lift(x1, x2, q1, q2) + big // 2) // big) % t


def row_words(n, k):
    return RNS_HEADER_WORDS + 2 * (k + 1) * n


def header(n, k, t, q1, q2):
    return [8 * (row_words(n, k) - 1), RNS_MAGIC, n | (k << 32), q1, q2, t]
