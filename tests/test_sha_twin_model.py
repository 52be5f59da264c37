"""CPU: the lane-pair round of sha256_twin_group (csrc/sha256.hip.h) written out on two-lane registers, against hashlib.

Every register is a pair [A, B]: lane A holds e, f, g, h and lane B holds a, b, c, d in the same four registers R0..R3.  One round
is the ten lane-pair instructions of the routine's comment block: three rotations by the lane's own amounts, the 3-input XOR
(0x96), D = x ^ (z & mask) (0x78, mask 0 on A and ~0 on B), the select (0xCA) — which is Ch on A and, through
Maj(a, b, c) = Ch(a ^ c, b, c), Maj on B —, the three-operand add with K + W on A and 0 on B, and the three exchange steps (a
masked add, a masked OR, an add with the partner's R3).  The Davies-Meyer add is four lane-pair adds.  This pins the truth
tables, the two shift triples and the identity; the kernel is checked on the GPU by tests/test_gpu_sha_twin.py."""
import hashlib
import itertools
import struct

import numpy as np

from test_gpu_sha_handover import BLOCKS_3_4_5, EDGE_LENS, nblk

M = 0xFFFFFFFF
K = [0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
     0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
     0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
     0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
     0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
     0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
     0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
     0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2]
IV = [0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19]

A, B = 0, 1
SH = ((6, 11, 25), (2, 13, 22))          # SHA_TWIN_SH: Σ1 on A, Σ0 on B
MASKB = (0, M)                           # SHA_TWIN_MASKB
LANE_OPS = [0]                           # lane-operations executed (two per lane-pair instruction)


def bitop3(a, b, c, table):
    """v_bitop3_b32: bit i of the result is bit (a_i << 2 | b_i << 1 | c_i) of the truth table"""
    out = 0
    for i in range(32):
        idx = ((a >> i) & 1) << 2 | ((b >> i) & 1) << 1 | ((c >> i) & 1)
        out |= ((table >> idx) & 1) << i
    return out


def alignbit(hi, lo, s):
    return (((hi << 32) | lo) >> (s & 31)) & M


def pairwise(f, *regs):
    """one instruction on both lanes of the pair"""
    LANE_OPS[0] += 2
    return [f(A, *(r[A] for r in regs)), f(B, *(r[B] for r in regs))]


def twin_round(R, kw):
    """R = [R0, R1, R2, R3], each [A, B]; kw = K[t] + W[t]"""
    R0, R1, R2, R3 = R
    r1 = pairwise(lambda l, x: alignbit(x, x, SH[l][0]), R0)
    r2 = pairwise(lambda l, x: alignbit(x, x, SH[l][1]), R0)
    r3 = pairwise(lambda l, x: alignbit(x, x, SH[l][2]), R0)
    S = pairwise(lambda l, x, y, z: bitop3(x, y, z, 0x96), r1, r2, r3)
    D = pairwise(lambda l, x, z: bitop3(x, z, MASKB[l], 0x78), R0, R2)
    F = pairwise(lambda l, d, y, z: bitop3(d, y, z, 0xCA), D, R1, R2)
    U = pairwise(lambda l, s, f: (s + f + (kw if l == A else 0)) & M, S, F)
    R3 = pairwise(lambda l, h, u: (h + u) & M if l == A else h, R3, U)          # bank-masked: A lanes only
    U = pairwise(lambda l, u, h: (0 | h) if l == A else u, U, R3)               # bank-masked: A lanes only
    partner = [R3[B], R3[A]]                                                    # row_half_mirror
    N = pairwise(lambda l, p, u: (p + u) & M, partner, U)
    return [N, R0, R1, R2]


def twin_sha256(msg: bytes) -> bytes:
    data = msg + b"\x80" + b"\x00" * ((55 - len(msg)) % 64) + struct.pack(">Q", 8 * len(msg))
    st = [[IV[4 + i], IV[i]] for i in range(4)]                                 # A: e..h, B: a..d
    for off in range(0, len(data), 64):
        w = list(struct.unpack(">16I", data[off:off + 64]))
        for t in range(16, 64):
            s0 = alignbit(w[t - 15], w[t - 15], 7) ^ alignbit(w[t - 15], w[t - 15], 18) ^ (w[t - 15] >> 3)
            s1 = alignbit(w[t - 2], w[t - 2], 17) ^ alignbit(w[t - 2], w[t - 2], 19) ^ (w[t - 2] >> 10)
            w.append((w[t - 16] + s0 + w[t - 7] + s1) & M)
        R = [list(r) for r in st]
        for t in range(64):
            R = twin_round(R, (K[t] + w[t]) & M)
        st = [pairwise(lambda l, x, y: (x + y) & M, st[i], R[i]) for i in range(4)]
    return struct.pack(">8I", *[st[i][B] for i in range(4)], *[st[i][A] for i in range(4)])


def test_truth_tables():
    for a, b, c in itertools.product((0, M), repeat=3):
        assert bitop3(a, b, c, 0x96) == a ^ b ^ c
        assert bitop3(a, b, c, 0x78) == a ^ (b & c)
        assert bitop3(a, b, c, 0xCA) == (a & b) | (~a & c & M)


def test_maj_is_ch_of_a_xor_c():
    rng = np.random.default_rng(1)
    for a, b, c in itertools.product((0, M), repeat=3):
        assert bitop3(a ^ c, b, c, 0xCA) == (a & b) | (a & c) | (b & c)
    for _ in range(64):
        a, b, c = (int(x) for x in rng.integers(0, 1 << 32, 3))
        assert bitop3(bitop3(a, c, M, 0x78), b, c, 0xCA) == (a & b) ^ (a & c) ^ (b & c)         # the B lane's D and F
        assert bitop3(bitop3(a, c, 0, 0x78), b, c, 0xCA) == (a & b) ^ (~a & c & M)              # the A lane's: Ch


def test_shift_triples():
    """FIPS 180-4 (4.4), (4.5): Σ0 = ROTR 2 ^ ROTR 13 ^ ROTR 22 on a (lane B), Σ1 = ROTR 6 ^ ROTR 11 ^ ROTR 25 on e (lane A)"""
    assert SH[B] == (2, 13, 22) and SH[A] == (6, 11, 25)
    x = 0x80000001
    assert alignbit(x, x, 1) == 0xC0000000 and alignbit(x, x, 31) == 0x00000003


def test_lane_pair_rounds_against_hashlib():
    rng = np.random.default_rng(2)
    for length in EDGE_LENS + BLOCKS_3_4_5:
        msg = rng.integers(0, 256, length, dtype=np.uint8).tobytes()
        LANE_OPS[0] = 0
        assert twin_sha256(msg) == hashlib.sha256(msg).digest(), length
        assert LANE_OPS[0] == nblk(length) * 2 * (64 * 10 + 4), length          # ten instructions per round, four for the state
