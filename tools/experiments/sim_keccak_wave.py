#!/usr/bin/env python3
"""CPU model of the wavefront-cooperative Keccak-f[1600] of lsr_keccak_wave.hpp: one 64-bit state word per hardware lane, lane
l = 5y + x of a 32-lane half holding A[x][y] (l < 25), the two halves of a wave64 hashing two messages at once.

The state is a 64-entry lane vector; every cross-lane move of the kernel (ds_bpermute) is the index permutation `v[src]` with
EXACTLY the lane table the kernel reads: the table is parsed out of lsr_keccak_wave.hpp (between LSR_KECCAK_WAVE_TABLE_BEGIN and
_END), not restated here.  `derive_table()` rebuilds the same table from FIPS 202 §3.2 (rho offsets, pi, the row/column neighbours)
and `check()` asserts that the header holds it and that the model reproduces hashlib.sha3_256.

  python tools/experiments/sim_keccak_wave.py          # check the header's table and the model
  python tools/experiments/sim_keccak_wave.py --emit   # print the table rows in the header's form"""
import hashlib
import os
import re
import sys

import numpy as np

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "lambda-snark-r_amd", "csrc", "lsr_keccak_wave.hpp")
COLUMNS = ["up5", "up10", "up15", "up20", "xm1", "xp1", "chi0", "chi1", "chi2", "rotr"]   # the first ten bytes of a table row
RATE = 136

# rho offsets r[x][y] (FIPS 202 §3.2.2, table 2)
RHO = [[0, 36, 3, 41, 18], [1, 44, 10, 45, 2], [62, 6, 43, 15, 61], [28, 55, 25, 21, 56], [27, 20, 39, 8, 14]]
RC = [0x0000000000000001, 0x0000000000008082, 0x800000000000808A, 0x8000000080008000, 0x000000000000808B, 0x0000000080000001,
      0x8000000080008081, 0x8000000000008009, 0x000000000000008A, 0x0000000000000088, 0x0000000080008009, 0x000000008000000A,
      0x000000008000808B, 0x800000000000008B, 0x8000000000008089, 0x8000000000008003, 0x8000000000008002, 0x8000000000000080,
      0x000000000000800A, 0x800000008000000A, 0x8000000080008081, 0x8000000000008080, 0x0000000080000001, 0x8000000080008008]


def derive_table():
    """[32][10] from the round function.  Lanes 25..31 of a half hold no state: they gather from themselves and never rotate."""
    pi_src = [0] * 25                    # B[y][2x + 3y] = rot(A[x][y]): the lane whose rotated word lands at lane 5Y + X
    for x in range(5):
        for y in range(5):
            pi_src[5 * ((2 * x + 3 * y) % 5) + y] = 5 * y + x
    rows = []
    for l in range(32):
        if l >= 25:
            rows.append([l] * 9 + [0])
            continue
        x, y = l % 5, l // 5
        row = [(l + k) % 25 for k in (5, 10, 15, 20)]                         # theta: the other four words of the column
        row += [5 * y + (x + 4) % 5, 5 * y + (x + 1) % 5]                     # theta: parity of columns x - 1 and x + 1
        row += [pi_src[5 * y + (x + d) % 5] for d in (0, 1, 2)]               # pi folded into chi's three operands
        row += [(64 - RHO[x][y]) % 64]                                         # rho as a right-rotate count
        rows.append(row)
    return rows


def header_table():
    text = open(HEADER).read()
    body = re.search(r"LSR_KECCAK_WAVE_TABLE_BEGIN(.*?)LSR_KECCAK_WAVE_TABLE_END", text, re.S).group(1)
    rows = [[int(v) for v in re.findall(r"\d+", m)] for m in re.findall(r"\{([^{}]*)\}", body)]
    assert len(rows) == 32 and all(len(r) == 16 for r in rows), "the header's table is [32][16]"
    return [r[:len(COLUMNS)] for r in rows]


class WaveModel:
    """Two sponges, one per 32-lane half, stepped together exactly as the kernel steps them."""

    def __init__(self, table=None):
        t = np.array(table if table is not None else header_table(), dtype=np.int64)
        lane = np.arange(64)
        half, l = lane & 32, lane & 31
        self.src = {name: half + t[l, i] for i, name in enumerate(COLUMNS[:9])}     # source LANE of every gather, both halves
        self.rotr = t[l, 9].astype(np.uint64)
        self.iota = (l == 0)

    @staticmethod
    def _rotl1(v):
        return (v << np.uint64(1)) | (v >> np.uint64(63))

    def round(self, a, rc):
        s = self.src
        c = a ^ a[s["up5"]] ^ a[s["up10"]] ^ a[s["up15"]] ^ a[s["up20"]]          # theta: every lane holds its column's parity
        a = a ^ c[s["xm1"]] ^ self._rotl1(c[s["xp1"]])
        r = (a >> self.rotr) | (a << ((np.uint64(64) - self.rotr) & np.uint64(63)))   # rho (a right rotate by 0 is the identity)
        r = np.where(self.rotr == 0, a, r)
        a = r[s["chi0"]] ^ (~r[s["chi1"]] & r[s["chi2"]])                           # pi and chi
        return a ^ np.where(self.iota, np.uint64(rc), np.uint64(0))                 # iota

    def permute(self, a):
        for rc in RC:
            a = self.round(a, rc)
        return a

    def sha3_256_pair(self, m0, m1):
        """SHA3-256 of two byte strings, one per half; the shorter one idles (absorbs nothing) once it is done."""
        a = np.zeros(64, dtype=np.uint64)
        out = [None, None]
        padded = []
        for m in (m0, m1):
            p = bytearray(m) + bytearray(RATE - len(m) % RATE)
            p[len(m)] ^= 0x06
            p[-1] ^= 0x80
            padded.append(np.frombuffer(bytes(p), dtype="<u8"))
        for blk in range(max(len(p) for p in padded) // 17):
            for h, p in enumerate(padded):
                if 17 * blk < len(p):
                    a[32 * h:32 * h + 17] ^= p[17 * blk:17 * blk + 17]
            a = self.permute(a)
            for h, p in enumerate(padded):
                if 17 * (blk + 1) == len(p):
                    out[h] = a[32 * h:32 * h + 4].astype("<u8").tobytes()
        return out


def check(messages=120, seed=1):
    assert header_table() == derive_table(), "lsr_keccak_wave.hpp's lane table is not the one FIPS 202 gives"
    model = WaveModel()
    rng = np.random.default_rng(seed)
    for i in range(messages // 2):
        ms = [rng.integers(0, 256, size=int(rng.integers(0, 601)), dtype=np.uint8).tobytes() for _ in range(2)]
        if i == 0:
            ms = [b"", bytes(range(136))]
        got = model.sha3_256_pair(*ms)
        for m, g in zip(ms, got):
            assert g == hashlib.sha3_256(m).digest(), len(m)
    return messages


if __name__ == "__main__":
    if "--emit" in sys.argv:
        for l, row in enumerate(derive_table()):
            print("    {" + ", ".join(f"{v:2d}" for v in row + [0] * 6) + "}," + (f"   // lane {l}: A[{l % 5}][{l // 5}]" if l < 25 else ""))
    else:
        print(f"table ok, {check()} messages equal hashlib.sha3_256")
