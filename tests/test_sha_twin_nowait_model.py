"""CPU: the round of sha256_twin_group's default build (csrc/sha256.hip.h, ZKE_SHA_TWIN_NOWAIT = 1) on lane-pair registers,
against hashlib, with the order of its instructions checked inside the model.

Registers are pairs [A, B] as in test_sha_twin_model.py (its tables and helpers are used, not copied).  One round is
  r1, r2, r3, S, D, F          as there
  W  = add3(S, F, Q)           Q: h + K + W on A, 0 on B
  N  = R3[partner] + W         all lanes; into the register of the dying R3
  Q' = Q' + R2                 A lanes only: the next round's Q, in place in its K + W register
  N  = W[partner] + W          B lanes only
and the claim of the scheme is that no wait state is needed: an instruction that reads a register through DPP — through the
partner, or with a bank mask — finds it written at least three instructions earlier (two stand between).  Every modelled
instruction therefore takes the next index of a block's stream and records it on the register it writes, and every such read
asserts the distance: the block-top Q (in front of round 0's add3) and round 63 (no next Q; one empty slot) included.  The state is
written by four moves at the top of the stream, R3 last, so the block-top Q's read of R3 is checked too; registers that come from LDS
(K + W) carry no write index.  The slot of a wait
state counts in the distance and is not a lane-pair instruction.  No assembly is looked at here."""
import hashlib
import struct

import numpy as np

import test_sha_twin_model as TM
from test_gpu_sha_handover import BLOCKS_3_4_5, EDGE_LENS, nblk
from test_sha_twin_model import A, B, IV, K, M, MASKB, SH, alignbit, bitop3

DPP_DISTANCE = 3          # a DPP read stands at least this many instructions behind the write of its register
MIN_SEEN = [None]         # the smallest distance a DPP read met


class Reg:
    """a lane-pair register and the stream index of the instruction that wrote it (None: it comes from LDS)"""

    def __init__(self, a, b, at=None):
        self.v = [a, b]
        self.at = at


class Stream:
    """the rounds wave's instruction stream of one block"""

    def __init__(self):
        self.pc = 0
        self.valu = 0
        self.per_round = [0] * 64

    def issue(self, f, *regs, dpp=(), lanes=(A, B), into=None, t=None):
        """One instruction on both lanes (`lanes`: the bank mask).  `dpp`: the operands read through DPP.  `t`: the round it
        belongs to (a Q belongs to the round that adds it, not to the one whose slot it fills)."""
        for r in dpp:
            if r.at is not None:
                dist = self.pc - r.at
                assert dist >= DPP_DISTANCE, f"instruction {self.pc} reads through DPP what instruction {r.at} wrote"
                MIN_SEEN[0] = dist if MIN_SEEN[0] is None else min(MIN_SEEN[0], dist)
        out = into if into is not None else Reg(0, 0)
        new = [f(l, *(r.v[l] for r in regs)) if l in lanes else out.v[l] for l in (A, B)]
        out.v, out.at = new, self.pc
        self.pc += 1
        self.valu += 1
        if t is not None:
            self.per_round[t] += 1
        TM.LANE_OPS[0] += 2
        return out

    def copy(self, r):
        """a move in front of the rounds (the state into R0..R3): takes a slot and writes its register; not one of the counted instructions"""
        out = Reg(r.v[A], r.v[B], self.pc)
        self.pc += 1
        return out

    def slot(self):
        """an issue slot with nothing in it (s_nop 0)"""
        self.pc += 1


def mirror(r):
    """the register as its partner lane sees it (row_half_mirror); shares the write index"""
    m = Reg(r.v[B], r.v[A], r.at)
    return m


def make_q(s, kw, r, t):
    """Q = Q + r on A lanes, for round t: r is read with a bank mask (an identity quad_perm)"""
    return s.issue(lambda l, q, x: (q + x) & M, kw, r, dpp=(r,), lanes=(A,), into=kw, t=t)


def nowait_round(s, R, kw, kw_next, t):
    """Round t on R = [R0, R1, R2, R3]; kw: its K + W register (Q already, unless t = 0); kw_next: round t + 1's, or None"""
    R0, R1, R2, R3 = R
    r1 = s.issue(lambda l, x: alignbit(x, x, SH[l][0]), R0, t=t)
    r2 = s.issue(lambda l, x: alignbit(x, x, SH[l][1]), R0, t=t)
    r3 = s.issue(lambda l, x: alignbit(x, x, SH[l][2]), R0, t=t)
    S = s.issue(lambda l, x, y, z: bitop3(x, y, z, 0x96), r1, r2, r3, t=t)
    D = s.issue(lambda l, x, z: bitop3(x, z, MASKB[l], 0x78), R0, R2, t=t)
    F = s.issue(lambda l, d, y, z: bitop3(d, y, z, 0xCA), D, R1, R2, t=t)
    if t == 0:
        make_q(s, kw, R3, 0)                                                # the block-top Q, in front of the first add3
    W = s.issue(lambda l, x, y, q: (x + y + q) & M, S, F, kw, t=t)
    N = s.issue(lambda l, p, w: (p + w) & M, mirror(R3), W, dpp=(R3,), into=R3, t=t)
    if kw_next is not None:
        make_q(s, kw_next, R2, t + 1)
    else:
        s.slot()                                                            # round 63: no next K + W
    N = s.issue(lambda l, p, w: (p + w) & M, mirror(W), W, dpp=(W,), lanes=(B,), into=N, t=t)
    return [N, R0, R1, R2]


def nowait_sha256(msg: bytes, counts=None) -> bytes:
    data = msg + b"\x80" + b"\x00" * ((55 - len(msg)) % 64) + struct.pack(">Q", 8 * len(msg))
    st = [[IV[4 + i], IV[i]] for i in range(4)]                             # A: e..h, B: a..d
    for off in range(0, len(data), 64):
        w = list(struct.unpack(">16I", data[off:off + 64]))
        for t in range(16, 64):
            s0 = alignbit(w[t - 15], w[t - 15], 7) ^ alignbit(w[t - 15], w[t - 15], 18) ^ (w[t - 15] >> 3)
            s1 = alignbit(w[t - 2], w[t - 2], 17) ^ alignbit(w[t - 2], w[t - 2], 19) ^ (w[t - 2] >> 10)
            w.append((w[t - 16] + s0 + w[t - 7] + s1) & M)
        s = Stream()
        kw = [Reg((K[t] + w[t]) & M, 0) for t in range(64)]                 # from LDS: B lanes read zeros
        # The state is written right in front of the rounds (the Davies-Meyer adds of the block before, then the copies into R0..R3),
        # R3 last, the order that leaves the block-top Q the least room: it reads R3 through DPP six instructions into round 0.
        R = first = [s.copy(Reg(*r)) for r in st]
        assert first[3].at == s.pc - 1 == 3
        for t in range(64):
            R = nowait_round(s, R, kw[t], kw[t + 1] if t < 63 else None, t)
            assert all(q.v[B] == 0 for q in kw)                             # Q stays 0 on B lanes
        assert s.per_round == [10] * 64 and s.valu == 640 and s.pc == 645   # exactly ten a round, round 63's empty slot, the four copies
        assert all(x is y for x, y in zip(R, first))                        # N went into the dying R3: no move, and after 64 rounds
        if counts is not None:                                              # every value is in its own register again
            counts.append((s.valu, s.pc))
        st = [TM.pairwise(lambda l, x, y: (x + y) & M, st[i], R[i].v) for i in range(4)]
    return struct.pack(">8I", *[st[i][B] for i in range(4)], *[st[i][A] for i in range(4)])


def test_rounds_against_hashlib_and_counts():
    rng = np.random.default_rng(2)
    for length in EDGE_LENS + BLOCKS_3_4_5:
        msg = rng.integers(0, 256, length, dtype=np.uint8).tobytes()
        TM.LANE_OPS[0] = 0
        counts = []
        assert nowait_sha256(msg, counts) == hashlib.sha256(msg).digest(), length
        assert TM.LANE_OPS[0] == nblk(length) * 2 * (64 * 10 + 4), length      # ten instructions per round, four for the state
        assert counts == [(640, 645)] * nblk(length)


def test_four_kb_message_and_carries():
    """A 4 096-byte message (65 blocks), and all-0x00 / all-0xFF blocks: carries out of h + K + W and out of the in-place add."""
    rng = np.random.default_rng(3)
    for msg in (rng.integers(0, 256, 4096, dtype=np.uint8).tobytes(), b"\x00" * 200, b"\xff" * 200):
        assert nowait_sha256(msg) == hashlib.sha256(msg).digest()


def test_every_dpp_read_is_three_instructions_behind_its_write():
    """The distance asserted in every issue() above is met with nothing to spare by W, and by nothing closer."""
    MIN_SEEN[0] = None
    nowait_sha256(b"abc" * 50)
    assert MIN_SEEN[0] == DPP_DISTANCE


def test_the_check_catches_the_old_exchange():
    """A DPP read two instructions behind the write of its register, the distance of the old exchange's last add, is refused."""
    s = Stream()
    W = s.issue(lambda l, x: x, Reg(1, 2))
    s.issue(lambda l, x: x, Reg(3, 4))
    try:
        s.issue(lambda l, p, w: (p + w) & M, mirror(W), W, dpp=(W,), lanes=(B,))
    except AssertionError:
        return
    raise AssertionError("a DPP read two instructions behind its write passed")
