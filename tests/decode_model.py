"""Pure-Python big-integer model of row decoding and the measured noise.  q is the modulus the coefficient lives under:
the context's prime, or Q = q1 q2 with x the CRT lift (rns_model.crt_lift) for an RNS context.  Nothing here touches the library."""


def slot_and_rho(x, t, q):
    """N = t x + floor(q/2) = s q + rem  ->  (slot = s mod t, rho = |rem - floor(q/2)| = |t x - s q|)"""
    half = q // 2
    s, rem = divmod(t * x + half, q)
    return (0 if s == t else s), abs(rem - half)


def noise_bits(xs, t, q):
    """bit length of the largest rho over the coefficients xs (0 when it is 0)"""
    return max(slot_and_rho(int(x), t, q)[1] for x in xs).bit_length()


def capacity_bits(q):
    return (q // 2).bit_length()


def centred(c, t):
    c %= t
    return c - t if c > t // 2 else c
