"""Big-integer model of the linear combination of commitment rows: what lsr_lwe_combine_rows_device must
compute, independently of any kernel."""


def centred(c, t):
    """the representative of c mod t in (-t/2, t/2]"""
    c %= t
    return c - t if c > t // 2 else c


def weight(coeffs, t):
    return sum(abs(centred(int(c), t)) for c in coeffs)


def combine(terms, coeffs, t, q):
    """sum_i centred(c_i) * terms[i][x] mod q for every x"""
    cs = [centred(int(c), t) for c in coeffs]
    return [sum(c * int(row[x]) for c, row in zip(cs, terms)) % q for x in range(len(terms[0]))]


def combine_rows(rows, coeffs, t, head, blocks):
    """wire rows (numpy uint64 [terms][words]) -> the combined row as a list of ints; blocks = [(first word, words, modulus)]"""
    out = [int(w) for w in rows[0][:head]] + [0] * (len(rows[0]) - head)
    for first, words, q in blocks:
        out[first:first + words] = combine([row[first:first + words].tolist() for row in rows], coeffs, t, q)
    return out
