"""Cases and expectations for the Ed25519 probe (tests/cpp/ed_probe.hip): the field, scalar, hash and point routines of
csrc/ed25519.hip.h driven one at a time, at the operands where a carry, a borrow or a second wrap can go wrong.

Expectations come from Python integers, hashlib and ed25519_ref only — never from the oracle or the device.  Field results
are compared modulo p (the kernel may return any 256-bit representative); fe_canon must return the value in [0, p) itself;
points are compared projectively.  The rare classes (CLASSES below) are value-level predicates on the 256-bit container,
not a restatement of the limb loops; tests/test_ed_field_cases.py checks on the CPU that every one of them selects a case.

Tape and result layout: see the head of tests/cpp/ed_probe.hip."""
import functools
import hashlib
import struct
from collections import namedtuple

import numpy as np

import ed25519_ref as ed
import ed_vectors

P, L, D = ed.P, ed.L, ed.D
M256 = 1 << 256
IN_WORDS, OUT_WORDS, HEADER_WORDS = 80, 40, 16
TAPE_MAGIC, RES_MAGIC = 0x42504445, 0x52504445

# op -> (code, family, operand widths in 32-bit words)
FE, PT = (8,), (8, 8, 8, 8)
OPS = {
    "fe_add": (1, 0, FE * 2), "fe_sub": (2, 0, FE * 2), "fe_mul": (3, 0, FE * 2), "fe_sq": (4, 0, FE),
    "fe_mul_i": (5, 0, FE * 2), "fe_sq_i": (6, 0, FE), "fe_canon": (7, 0, FE), "fe_is_zero": (8, 0, FE),
    "fe_eq": (9, 0, FE * 2), "fe_is_neg": (10, 0, FE), "fe_neg": (11, 0, FE), "fe_invert": (12, 0, FE),
    "fe_pow22523": (13, 0, FE), "fe_from_bytes": (14, 0, FE),
    "sc_lt_L": (20, 1, FE), "sc_reduce512": (21, 1, (16,)), "sha512_ram": (22, 1, FE * 3),
    "ge_decompress": (30, 2, FE), "ge_compress": (31, 2, PT), "ge_is_small_order": (32, 2, PT),
    "ge_add": (33, 2, PT * 2), "ge_dbl": (34, 2, PT), "ge_add_cached": (35, 2, PT * 2 + FE),
    "q_table": (40, 3, PT), "q_dbl": (41, 3, PT), "q_add": (42, 3, PT * 2),
}
CODE_TO_OP = {v[0]: k for k, v in OPS.items()}

# ins: a flat tuple of Python ints, one per operand of OPS[op][2]; aux: the record's second word (sha512_ram: mlen);
# exp: the expectation, whose meaning depends on the op (see check())
Case = namedtuple("Case", "op ins aux exp")


def _rng(seed):
    return np.random.default_rng(seed)


def _rand(rng, bits=256):
    return int.from_bytes(rng.integers(0, 256, (bits + 7) // 8, dtype=np.uint8).tobytes(), "little") & ((1 << bits) - 1)


# ---------------------------------------------------------------------------------------------- field operands
def field_pool():
    """The ~100 containers every binary op sees in all ordered pairs."""
    v = [0, 1, 2, 18, 19, 20, 37, 38, 39]
    v += [P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, 2 ** 255 - 1, 2 ** 255]
    v += [M256 - k for k in range(39, 0, -1)]
    for k in range(1, 8):
        v += [1 << (32 * k), (1 << (32 * k)) - 1, M256 - (1 << (32 * k))]
    for k in range(8):
        v += [M256 - 1 - (0xffffffff << (32 * k)), 0xffffffff << (32 * k)]      # one limb cleared; one limb set
    v += [D, 2 * D % P, ed.SQRT_M1]
    rng = _rng(101)
    v += [_rand(rng) for _ in range(4)]
    return list(dict.fromkeys(v))


def invert_subset():
    rng = _rng(102)
    v = [0, 1, 2, 19, 38, P - 1, P, P + 1, 2 * P, 2 ** 255, M256 - 1, D, ed.SQRT_M1] + [_rand(rng) for _ in range(3)]
    assert len(v) == 16
    return v


def add_rare_pairs():
    rng = _rng(103)
    out = [(M256 - 1, M256 - 1), (M256 - 1, M256 - 38), (M256 - 19, M256 - 19)]       # carry, and the 38 wraps again
    for _ in range(4):
        a = _rand(rng)
        out += [(a, M256 - 1 - a), (a, M256 - a)]                                      # sum 2^256 - 1; sum 2^256
    out += [(1 << 255, 1 << 255), (0, M256 - 1)]
    return out


def sub_rare_pairs():
    rng = _rng(104)
    out = [(0, M256 - 1), (5, M256 - 20), (36, M256 - 1), (0, M256 - 37)]             # borrow, and the 38 borrows again
    for _ in range(4):
        a = _rand(rng) | 1 << 200
        out += [(a, a), (a - 1, a)]
    out += [(0, 1), (M256 - 2, M256 - 1)]
    return out


def mul_terms(a, b):
    """F = lo + 38 hi of the 512-bit product, and its part above 2^256."""
    t = a * b
    F = (t % M256) + 38 * (t >> 256)
    return F, F >> 256


def is_second_wrap(a, b):
    F, c = mul_terms(a, b)
    return (F % M256) + 38 * c >= M256


C_MAX = mul_terms(M256 - 1, M256 - 1)[1]


def mul_second_wrap_pairs(count=48):
    """a odd and prime to p, b = e / a mod 2p with 38 <= e <= 75: F = e (mod 2p), so folding F's top word back in lands on
    e or e + 2p = e + 2^256 - 38 >= 2^256.  The pairs where it does are kept."""
    rng = _rng(105)
    out = []
    while len(out) < count:
        a = _rand(rng) | 1
        if a % P == 0:
            continue
        e = 38 + int(rng.integers(0, 38))
        b = e * pow(a, -1, 2 * P) % (2 * P)
        if is_second_wrap(a, b):
            out.append((a, b))
    return out


def sq_second_wrap_operands():
    """square roots of e < 200 mod p, lifted by p where needed so that a^2 = e (mod 2p); those that wrap twice are kept"""
    out = []
    for e in range(38, 200):
        r = pow(e, (P + 3) // 8, P)
        if r * r % P != e:
            r = r * ed.SQRT_M1 % P
        if r * r % P != e:
            continue                                   # not a square
        for a in (r, P - r):
            if (a ^ e) & 1:
                a += P
            assert a * a % (2 * P) == e
            if is_second_wrap(a, a):
                out.append(a)
    return out


def canon_operands():
    rng = _rng(106)
    lo = [_rand(rng, 254) for _ in range(3)]
    return lo + [P + x for x in lo] + [2 * P + k for k in (0, 1, 7, 18)] + [M256 - k for k in (19, 10, 1)] + \
        [M256 - 20, M256 - 38, 2 * P - 1, P - 1, P, 0]


_CANON_TWINS = frozenset(canon_operands()[:6])          # three random x < 2^254 and their x + p


def predicate_operands():
    return [0, 1, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, 38, 37, 39, 19, M256 - 1, 2 ** 255 - 19, 2 ** 255, D]


# ---------------------------------------------------------------------------------------------- rare classes
def _busy(x):
    return all(0 < (x >> (32 * k)) & 0xffffffff < 0xffffffff for k in range(8))


CLASSES = {
    # name: predicate on a Case
    "add: carry out and the folded 38 wraps again": lambda c: c.op == "fe_add" and sum(c.ins) >= M256 and sum(c.ins) % M256 + 38 >= M256,
    "add: a+b = 2^256-1": lambda c: c.op == "fe_add" and sum(c.ins) == M256 - 1,
    "add: a+b = 2^256": lambda c: c.op == "fe_add" and sum(c.ins) == M256,
    "sub: borrow and the 38 borrows again": lambda c: c.op == "fe_sub" and c.ins[0] < c.ins[1] and c.ins[0] - c.ins[1] + M256 < 38,
    "sub: a = b": lambda c: c.op == "fe_sub" and c.ins[0] == c.ins[1],
    "sub: a-b = -1": lambda c: c.op == "fe_sub" and c.ins[0] - c.ins[1] == -1,
    "neg: the second borrow": lambda c: c.op == "fe_neg" and 0 < M256 - c.ins[0] < 38,
    # the same sums and differences on operands with no limb of zeros or ones: the carry runs through real data
    "add: a+b = 2^256-1, busy limbs": lambda c: c.op == "fe_add" and sum(c.ins) == M256 - 1 and all(map(_busy, c.ins)),
    "add: a+b = 2^256, busy limbs": lambda c: c.op == "fe_add" and sum(c.ins) == M256 and all(map(_busy, c.ins)),
    "sub: a = b, busy limbs": lambda c: c.op == "fe_sub" and c.ins[0] == c.ins[1] and _busy(c.ins[0]),
    "sub: a-b = -1, busy limbs": lambda c: c.op == "fe_sub" and c.ins[0] - c.ins[1] == -1 and all(map(_busy, c.ins)),
}
for _op in ("fe_mul", "fe_mul_i", "fe_sq", "fe_sq_i"):
    _two = _op in ("fe_mul", "fe_mul_i")
    _ab = (lambda c: c.ins) if _two else (lambda c: (c.ins[0], c.ins[0]))
    CLASSES[_op + ": c = 0"] = lambda c, o=_op, ab=_ab: c.op == o and mul_terms(*ab(c))[1] == 0
    CLASSES[_op + ": c maximal"] = lambda c, o=_op, ab=_ab: c.op == o and mul_terms(*ab(c))[1] == C_MAX
    CLASSES[_op + ": second wrap"] = lambda c, o=_op, ab=_ab: c.op == o and is_second_wrap(*ab(c))
    CLASSES[_op + ": second wrap, busy limbs"] = lambda c, o=_op, ab=_ab: c.op == o and all(map(_busy, c.ins)) and len(set(c.ins)) == len(c.ins) and is_second_wrap(*ab(c))   # and a != b
_RANGES = {"[0,p)": (0, P), "[p,2p)": (P, 2 * P), "[2p,2^256)": (2 * P, M256), "[2^256-19,2^256)": (M256 - 19, M256)}
# classes that need at least this many cases
CLASS_MIN = {}
for _name, (_lo, _hi) in _RANGES.items():
    CLASSES["canon: " + _name] = lambda c, lo=_lo, hi=_hi: c.op == "fe_canon" and lo <= c.ins[0] < hi
    CLASS_MIN["canon: " + _name] = 3
CLASSES["canon: x and x+p, busy limbs"] = lambda c: c.op == "fe_canon" and c.ins[0] in _CANON_TWINS and _busy(c.ins[0])
CLASS_MIN["canon: x and x+p, busy limbs"] = 6
for _op in ("fe_is_zero", "fe_is_neg"):
    for _v in (0, P, 2 * P):
        for _d in (-1, 0, 1):
            if _v + _d >= 0:
                CLASSES["%s: %#x%+d" % (_op, _v, _d)] = lambda c, o=_op, x=_v + _d: c.op == o and c.ins[0] == x
    CLASSES[_op + ": 38"] = lambda c, o=_op: c.op == o and c.ins[0] == 38
CLASSES["eq: x, x+p"] = lambda c: c.op == "fe_eq" and c.ins[1] - c.ins[0] == P
CLASSES["eq: x, x+2p"] = lambda c: c.op == "fe_eq" and c.ins[1] - c.ins[0] == 2 * P
CLASSES["eq: x+2p, x"] = lambda c: c.op == "fe_eq" and c.ins[0] - c.ins[1] == 2 * P
CLASSES["eq: unequal neighbours"] = lambda c: c.op == "fe_eq" and abs(c.ins[0] - c.ins[1]) == 1
CLASSES["sc_lt_L: equal to L in the top five limbs, below"] = lambda c: c.op == "sc_lt_L" and c.ins[0] >> 96 == L >> 96 and c.ins[0] < L
CLASSES["sc_lt_L: equal to L in the top five limbs, above"] = lambda c: c.op == "sc_lt_L" and c.ins[0] >> 96 == L >> 96 and c.ins[0] > L
CLASSES["sc_lt_L: L"] = lambda c: c.op == "sc_lt_L" and c.ins[0] == L
CLASSES["sc_reduce512: a multiple of L"] = lambda c: c.op == "sc_reduce512" and c.ins[0] > 0 and c.ins[0] % L == 0
CLASSES["sc_reduce512: one below a multiple of L"] = lambda c: c.op == "sc_reduce512" and c.ins[0] % L == L - 1
CLASSES["sc_reduce512: 2^512-1"] = lambda c: c.op == "sc_reduce512" and c.ins[0] == 2 ** 512 - 1
for _m in range(1, 33):
    CLASSES["sha512_ram: mlen %d" % _m] = lambda c, m=_m: c.op == "sha512_ram" and c.aux == m
CLASSES["decompress: not a point"] = lambda c: c.op == "ge_decompress" and c.exp is None
CLASSES["decompress: y >= p"] = lambda c: c.op == "ge_decompress" and c.ins[0] % 2 ** 255 >= P
CLASSES["decompress: x = 0 with the sign bit"] = lambda c: c.op == "ge_decompress" and c.exp is not None and c.exp[0] == 0 and c.ins[0] >> 255
CLASSES["compress: Z != 1"] = lambda c: c.op == "ge_compress" and c.ins[2] % P != 1
for _op in ("ge_add", "ge_add_cached", "q_add"):
    CLASSES[_op + ": doubling by addition"] = lambda c, o=_op: c.op == o and _same_point(c.ins[0:4], c.ins[4:8]) and not ed.is_small_order(_aff(c.ins[0:4]))
    CLASSES[_op + ": P + (-P)"] = lambda c, o=_op: c.op == o and _same_point(c.ins[0:4], ed.neg(c.ins[4:8])) and not ed.is_small_order(_aff(c.ins[0:4]))
    CLASSES[_op + ": identity on the left"] = lambda c, o=_op: c.op == o and ed.is_identity(c.ins[0:4]) and not ed.is_identity(c.ins[4:8])
    CLASSES[_op + ": identity on the right"] = lambda c, o=_op: c.op == o and ed.is_identity(c.ins[4:8]) and not ed.is_identity(c.ins[0:4])
    CLASSES[_op + ": torsion + torsion"] = lambda c, o=_op: c.op == o and all(ed.is_small_order(_aff(x)) and not ed.is_identity(x) for x in (c.ins[0:4], c.ins[4:8]))
    CLASSES[_op + ": unreduced coordinates"] = lambda c, o=_op: c.op == o and all(x >= P for x in c.ins[0:8])
for _op in ("ge_dbl", "q_dbl"):
    CLASSES[_op + ": identity"] = lambda c, o=_op: c.op == o and ed.is_identity(c.ins[0:4])
    CLASSES[_op + ": torsion"] = lambda c, o=_op: c.op == o and ed.is_small_order(_aff(c.ins[0:4])) and not ed.is_identity(c.ins[0:4])
    CLASSES[_op + ": unreduced coordinates"] = lambda c, o=_op: c.op == o and all(x >= P for x in c.ins[0:4])


def _aff(pt):
    zi = pow(pt[2], P - 2, P)
    x, y = pt[0] * zi % P, pt[1] * zi % P
    return (x, y, 1, x * y % P)


def _same_point(a, b):
    return (a[0] * b[2] - b[0] * a[2]) % P == 0 and (a[1] * b[2] - b[1] * a[2]) % P == 0


# ---------------------------------------------------------------------------------------------- points
def affine_add(a, b):
    """The affine addition law of -x^2 + y^2 = 1 + d x^2 y^2, independent of the extended-coordinate formulas."""
    (x1, y1), (x2, y2) = a[:2], b[:2]
    k = D * x1 * x2 * y1 * y2 % P
    x3 = (x1 * y2 + x2 * y1) * pow(1 + k, P - 2, P) % P
    y3 = (y1 * y2 + x1 * x2) * pow(1 - k, P - 2, P) % P
    return (x3, y3, 1, x3 * y3 % P)


def on_curve(pt):
    X, Y, Z, T = (v % P for v in pt)
    return Z != 0 and (-X * X + Y * Y - Z * Z - D * T * T) % P == 0 and (X * Y - Z * T) % P == 0


def _lift(v):
    return v + 2 * P if v + 2 * P < M256 else v + P


def present(pt, mode, rng):
    """An affine point in one of three coordinate presentations: as it is; times a random Z; on unreduced representatives
    (x + 2p where that fits 256 bits — the 0 and 1 of the identity and of the torsion points — else x + p)."""
    if mode == "affine":
        return tuple(pt)
    lam = 1 if (mode == "lifted" and ed.is_small_order(pt)) else 2 + _rand(rng, 250)
    out = tuple(v * lam % P for v in pt)
    return tuple(_lift(v) for v in out) if mode == "lifted" else out


MODES = ("affine", "lambda", "lifted")


@functools.lru_cache(maxsize=None)
def points():
    rng = _rng(201)
    Pl = _aff(ed.mul(_rand(rng, 250) | 1, ed.BASE))
    tors = [_aff(t) for t in ed_vectors.torsion_points()]
    rnd = [_aff(ed.mul(_rand(rng, 250), ed.BASE)) for _ in range(4)]
    return {"P": Pl, "B": _aff(ed.BASE), "O": ed.IDENT, "T": tors, "R": rnd}


def point_pairs():
    z = points()
    Pl, B, O, T, R = z["P"], z["B"], z["O"], z["T"], z["R"]
    pairs = [(Pl, Pl), (Pl, _aff(ed.neg(Pl))), (Pl, O), (O, Pl), (O, O), (B, B), (B, Pl), (Pl, B), (B, _aff(ed.neg(B)))]
    pairs += [(a, b) for a in T for b in T]
    pairs += [(Pl, affine_add(Pl, t)) for t in T]
    pairs += [(R[0], R[1]), (R[2], R[3]), (R[1], R[0]), (R[3], Pl)]
    return pairs


def point_singles():
    z = points()
    return [z["P"], z["B"], z["O"]] + z["T"] + [affine_add(z["P"], t) for t in z["T"][1:]] + z["R"]


def decompress_inputs():
    enc = []
    for k, _, s, _ in ed_vectors.build_vectors():
        enc += [k, s[:32]]
    for y in (0, 1, P - 1, P, P + 1, 2 ** 255 - 1):
        for sgn in (0, 1):
            enc.append((y | sgn << 255).to_bytes(32, "little"))
    return list(dict.fromkeys(enc))


# ---------------------------------------------------------------------------------------------- scalars, hash
def sc_lt_inputs():
    v = [L, L - 1, L + 1, 0, 2 ** 252, M256 - 1]
    for k in range(8):
        limb = (L >> (32 * k)) & 0xffffffff
        if limb != 0xffffffff:
            v.append(L + (1 << (32 * k)))
        v.append(L - (1 << (32 * k)))
        if not limb:
            v.append(L | (0xffffffff << (32 * k)))       # a zero limb "decremented" alone wraps to all-ones
    rng = _rng(301)
    top = L >> 96 << 96
    v += [top | _rand(rng, 96) for _ in range(6)] + [top, top | (2 ** 96 - 1)]
    return v


def sc_reduce_inputs():
    rng = _rng(302)
    v = [0, L - 1, L, L + 1] + [1 << i for i in range(512)] + [2 ** 512 - 1]
    for m in [1, 2 ** 512 // L] + [_rand(rng, 258) + 1 for _ in range(16)]:
        v += [m * L, m * L - 1]
    v += [_rand(rng, 512) for _ in range(64)]
    assert all(0 <= x < 2 ** 512 for x in v)
    return v


def sha_inputs():
    rng = _rng(303)
    out = []
    for mlen in range(1, 33):
        R, A, M = (_rand(rng) for _ in range(3))        # all 32 message bytes are random: only mlen of them are hashed
        out.append((R, A, M, mlen))
    for mlen in (1, 15, 16, 17, 31, 32):
        out.append((M256 - 1, M256 - 1, M256 - 1, mlen))
    return out


# ---------------------------------------------------------------------------------------------- the case list
@functools.lru_cache(maxsize=None)
def build_cases():
    """-> tuple of Case, grouped by family in the order the tape wants (field, scalar and hash, points, quads)."""
    c = []
    pool = field_pool()

    def fe2(op, a, b, exp):
        c.append(Case(op, (a, b), 0, exp))

    pairs = [(a, b) for a in pool for b in pool]
    for a, b in pairs + add_rare_pairs():
        fe2("fe_add", a, b, (a + b) % P)
    for a, b in pairs + sub_rare_pairs():
        fe2("fe_sub", a, b, (a - b) % P)
    sq_ops = pool + sq_second_wrap_operands() + canon_operands()
    for op in ("fe_mul", "fe_mul_i"):
        for a, b in pairs + mul_second_wrap_pairs() + [(a, a) for a in sq_second_wrap_operands()[:16]]:
            fe2(op, a, b, a * b % P)
    for op in ("fe_sq", "fe_sq_i"):
        for a in sq_ops:
            c.append(Case(op, (a,), 0, a * a % P))
    unary = list(dict.fromkeys(pool + canon_operands() + predicate_operands()))
    for a in unary:
        c.append(Case("fe_canon", (a,), 0, a % P))
        c.append(Case("fe_is_zero", (a,), 0, int(a % P == 0)))
        c.append(Case("fe_is_neg", (a,), 0, a % P & 1))
        c.append(Case("fe_neg", (a,), 0, -a % P))
        c.append(Case("fe_from_bytes", (a,), 0, (a & (2 ** 255 - 1)) % P))
    pv = predicate_operands()
    eq = [(a, b) for a in pv for b in pv]
    for x in pv + pool[-8:]:
        eq += [(x, x)] + [(x, x + k) for k in (P, 2 * P, 1) if x + k < M256] + [(x + k, x) for k in (P, 2 * P) if x + k < M256]
    for a, b in dict.fromkeys(eq):
        fe2("fe_eq", a, b, int((a - b) % P == 0))
    for a in invert_subset():
        c.append(Case("fe_invert", (a,), 0, pow(a, P - 2, P)))
        c.append(Case("fe_pow22523", (a,), 0, pow(a, 2 ** 252 - 3, P)))

    for s in sc_lt_inputs():
        c.append(Case("sc_lt_L", (s,), 0, int(s < L)))
    for h in sc_reduce_inputs():
        c.append(Case("sc_reduce512", (h,), 0, h % L))
    for R, A, M, mlen in sha_inputs():
        msg = b"".join(x.to_bytes(32, "little") for x in (R, A)) + M.to_bytes(32, "little")[:mlen]
        c.append(Case("sha512_ram", (R, A, M), mlen, int.from_bytes(hashlib.sha512(msg).digest(), "little")))

    for enc in decompress_inputs():
        c.append(Case("ge_decompress", (int.from_bytes(enc, "little"),), 0, ed.decompress(enc)))
    rng = _rng(202)
    for pt in point_singles():
        for mode in MODES:
            q = present(pt, mode, rng)
            c.append(Case("ge_compress", q, 0, int.from_bytes(ed.compress(pt), "little")))
            c.append(Case("ge_is_small_order", q, 0, int(ed.is_small_order(pt))))
            c.append(Case("ge_dbl", q, 0, affine_add(pt, pt)))
            c.append(Case("q_dbl", q, 0, affine_add(pt, pt)))
            c.append(Case("q_table", q, 0, ((q[1] - q[0]) % P, (q[1] + q[0]) % P, 2 * D * q[3] % P, q[2] % P)))
    for a, b in point_pairs():
        for mode in MODES:
            pa, pb = present(a, mode, rng), present(b, mode, rng)
            exp = affine_add(a, b)
            t2d = 2 * D * pb[3] % P
            c.append(Case("ge_add", pa + pb, 0, exp))
            c.append(Case("ge_add_cached", pa + pb + (_lift(t2d) if mode == "lifted" else t2d,), 0, exp))
            c.append(Case("q_add", pa + pb, 0, exp))
    c.sort(key=lambda k: (OPS[k.op][1], OPS[k.op][0]))          # stable: families contiguous, ops grouped within them
    return tuple(c)


# ---------------------------------------------------------------------------------------------- tape
def _words(value, nwords):
    return int(value).to_bytes(4 * nwords, "little")


def pack_tape(cases) -> bytes:
    fam = [[None, 0] for _ in range(4)]
    body = bytearray()
    for i, k in enumerate(cases):
        code, f, widths = OPS[k.op]
        if fam[f][0] is None:
            fam[f][0] = i
        assert fam[f][0] + fam[f][1] == i, "the records of a family are contiguous"
        fam[f][1] += 1
        assert len(k.ins) == len(widths)
        rec = struct.pack("<II", code, k.aux) + b"".join(_words(v, w) for v, w in zip(k.ins, widths))
        body += rec.ljust(4 * IN_WORDS, b"\0")
    hd = [TAPE_MAGIC, len(cases), IN_WORDS, OUT_WORDS] + [x for s, n in fam for x in (s or 0, n)] + [0] * 4
    return struct.pack("<%dI" % HEADER_WORDS, *hd) + bytes(body)


def unpack_tape(tape: bytes):
    """-> list of (op, ins, aux): what pack_tape wrote, read back"""
    hd = struct.unpack_from("<%dI" % HEADER_WORDS, tape)
    assert hd[0] == TAPE_MAGIC and hd[2] == IN_WORDS and hd[3] == OUT_WORDS
    assert len(tape) == 4 * (HEADER_WORDS + hd[1] * IN_WORDS)
    out = []
    for i in range(hd[1]):
        rec = tape[4 * (HEADER_WORDS + i * IN_WORDS):4 * (HEADER_WORDS + (i + 1) * IN_WORDS)]
        code, aux = struct.unpack_from("<II", rec)
        op = CODE_TO_OP[code]
        ins, off = [], 8
        for w in OPS[op][2]:
            ins.append(int.from_bytes(rec[off:off + 4 * w], "little"))
            off += 4 * w
        assert not any(rec[off:])
        out.append((op, tuple(ins), aux))
    return out, hd


def unpack_results(blob: bytes, n: int):
    """-> an (n, OUT_WORDS) array of the probe's result words"""
    hd = struct.unpack_from("<4I", blob)
    assert hd[0] == RES_MAGIC and hd[1] == n and hd[2] == OUT_WORDS, hd
    assert len(blob) == 16 + 4 * n * OUT_WORDS
    return np.frombuffer(blob, "<u4", offset=16).reshape(n, OUT_WORDS)


# ---------------------------------------------------------------------------------------------- checking a result
def _int(words):
    return int.from_bytes(np.asarray(words, "<u4").tobytes(), "little")


def _hex(vals):
    return " ".join("%#x" % v for v in vals)


def check(case: Case, row):
    """None when the probe's result row answers the case, else a message naming the op, operands and result in hex."""
    op, exp = case.op, case.exp
    flag, fe = int(row[0]), [_int(row[1 + 8 * k:9 + 8 * k]) for k in range(4)]

    def bad(got, want):
        return "%s(%s)%s: got %s, expected %s" % (op, _hex(case.ins), " aux=%d" % case.aux if case.aux else "", got, want)

    if op in ("fe_is_zero", "fe_eq", "fe_is_neg", "sc_lt_L", "ge_is_small_order"):
        return None if flag == exp else bad(flag, exp)
    if op == "fe_canon":
        return None if fe[0] == exp else bad(hex(fe[0]), hex(exp) + " exactly")
    if op in ("sc_reduce512", "ge_compress"):
        return None if fe[0] == exp else bad(hex(fe[0]), hex(exp))
    if op == "sha512_ram":
        got = _int(row[1:17])
        return None if got == exp else bad(hex(got), hex(exp))
    if OPS[op][1] == 0:
        return None if fe[0] % P == exp else bad(hex(fe[0]), hex(exp) + " mod p")
    if op == "ge_decompress":
        if exp is None:
            return None if flag == 0 else bad("ok", "not a point")
        # affine: the verification reads X and Y as x and y
        ok = flag == 1 and [v % P for v in fe] == [exp[0], exp[1], 1, exp[3]]
        return None if ok else bad("ok=%d %s" % (flag, _hex(fe)), _hex(exp) + " mod p")
    if op == "q_table":
        return None if tuple(v % P for v in fe) == exp else bad(_hex(fe), _hex(exp) + " mod p")
    X, Y, Z, T = fe
    Xr, Yr, Zr, _ = exp
    ok = Z % P != 0 and (X * Zr - Xr * Z) % P == 0 and (Y * Zr - Yr * Z) % P == 0 and (T * Z - X * Y) % P == 0
    return None if ok else bad(_hex(fe), "the point " + _hex(exp) + " projectively")
