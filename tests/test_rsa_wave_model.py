"""CPU (-m "not gpu"): a model of the one-signature-per-wave RSA routine (csrc/rsa.hip.h mont_core_64 / mont_core_128,
big_normalize, big_ge, big_sub, mod_double; csrc/rsa_kernel.hip.h rsa_wave) step for step, one numpy element per 32-bit
limb (limb q*64 + lane), with the routine's carries kept where the instructions keep them; and the coverage the edge
cases of tests/rsa_edge_cases.py give to it and to the lane-group model of tests/test_rsa_group_model.py.

Each CIOS step of mont_core_64 / 128, per limb j (T = tl + th 2^32 is the 64-bit addend of the first multiply):
  P = a_j b_i + T              carry-out c0 (the 65th bit)
  m = lo(P_0) ninv             (limb 0 = lane 0 of the lower group)
  Q = n_j m + P                carry-out c1
  tl' = hi(Q_j) + lo(Q_j+1)    carry c2; limb 64 (lane 0 of the upper group) reaches limb 63 through the lane-63 hand-off
  th' = c0 + c1 + c2
The models must equal pow(s, e, n) on the case set, and the cases must make the data-dependent paths happen: c0 for one
and two limbs per lane, a carry out of the lane-63 hand-off, the `top != 0` subtraction, and for the lane-group routine
the final subtraction with a borrow into every lane 1..G-1 and the s >= n check decided by every lane of a group."""
import random
from collections import Counter

import numpy as np
import pytest

import rsa_edge_cases as rc
import synth
import test_rsa_group_model as gm

M32 = 0xFFFFFFFF
U64 = np.uint64


def limbs(x, NL):
    return np.array([(x >> (32 * j)) & M32 for j in range(64 * NL)], dtype=U64)


def value(v):
    return sum(int(l) << (32 * j) for j, l in enumerate(v))


def lanes_of(v, q):
    return v[64 * q:64 * (q + 1)]


def mont_core(a, b, n, ninv, cov):
    """mont_core_64 (64 limbs) / mont_core_128 (128): -> (tl, th) columns after 64 NL steps"""
    L = len(a)
    tl = np.zeros(L, dtype=U64)
    th = np.zeros(L, dtype=U64)
    for i in range(L):
        T = tl + (th << U64(32))
        P0 = a * b[i]                                            # < 2^64: no wrap
        P = P0 + T                                               # v_mad_u64_u32: 64-bit sum, carry-out c0
        c0 = (P < P0).astype(U64)
        m = U64((int(P[0]) & M32) * ninv & M32)
        Q0 = n * m
        Q = Q0 + P
        c1 = (Q < Q0).astype(U64)
        lo, hi = Q & U64(M32), Q >> U64(32)
        assert lo[0] == 0                                        # limb 0 is reduced by the quotient digit
        nxt = np.append(lo[1:], U64(0))                          # wave_shl:1; NL = 2: limb 64 -> limb 63 is the hand-off
        s = hi + nxt
        c2 = (s > U64(M32)).astype(U64)
        tl = s & U64(M32)
        th = c0 + c1 + c2
        if c0.any():
            cov["c0", L // 64] += 1
        if L == 128 and c2[63]:
            cov["handoff"] += 1                                  # tl' of lane 63 (lower group) overflowed with limb 64's word
        assert th.max() <= 3
    return tl, th


def ballot(pred):
    return sum(1 << l for l in range(64) if pred[l])


def big_normalize(tl, th, cov):
    """columns -> 32-bit limbs by the ballot carry-lookahead of big_normalize; -> (limbs, overflow word)"""
    NL = len(tl) // 64
    r = np.zeros_like(tl)
    cin, cbit = 0, 0
    for q in range(NL):
        lo, hi = lanes_of(tl, q), lanes_of(th, q)
        up = np.concatenate(([U64(cin)], hi[:-1]))               # hi of limb - 1; lane 0 gets the previous group's lane 63
        x = (lo + up) & U64(M32)
        g, p = ballot(x < up), ballot(x == U64(M32))
        gs = ((g << 1) & ((1 << 64) - 1)) | cbit
        sm = (gs + p) & ((1 << 64) - 1)
        cout = (g >> 63) | (1 if sm < gs else 0)
        inc = sm ^ p
        r[64 * q:64 * (q + 1)] = (x + np.array([(inc >> l) & 1 for l in range(64)], dtype=U64)) & U64(M32)
        if q == 0 and NL == 2 and (int(hi[63]) or cout):
            cov["normalize-crosses-groups"] += 1
        cin, cbit = int(hi[63]), cout
    return r, cin + cbit


def big_ge(x, y):
    NL = len(x) // 64
    for q in reversed(range(NL)):
        gt, lt = ballot(lanes_of(x, q) > lanes_of(y, q)), ballot(lanes_of(x, q) < lanes_of(y, q))
        if gt != lt:
            return gt > lt
    return True


def big_sub(x, y):
    """x - y mod 2^(2048 NL) by the ballot borrow-lookahead; -> (r, borrow out)"""
    NL = len(x) // 64
    r = np.zeros_like(x)
    b = 0
    for q in range(NL):
        xq, yq = lanes_of(x, q), lanes_of(y, q)
        d = (xq - yq) & U64(M32)
        g, p = ballot(xq < yq), ballot(d == U64(0))
        gs = ((g << 1) & ((1 << 64) - 1)) | b
        sm = (gs + p) & ((1 << 64) - 1)
        cout = (g >> 63) | (1 if sm < gs else 0)
        inc = sm ^ p
        r[64 * q:64 * (q + 1)] = (d - np.array([(inc >> l) & 1 for l in range(64)], dtype=U64)) & U64(M32)
        b = cout
    return r, b


def mont_mul(a, b, n, ninv, cov):
    tl, th = mont_core(a, b, n, ninv, cov)
    t, top = big_normalize(tl, th, cov)
    if top:
        cov["top", len(a) // 64] += 1
    if top or big_ge(t, n):
        return big_sub(t, n)[0]
    return t


def mod_double(x, n, cov):
    d = ((x << U64(1)) | np.concatenate(([U64(0)], x[:-1] >> U64(31)))) & U64(M32)    # lane 0 of group 1: lane 63's bit
    top = int(x[-1]) >> 31
    if top:
        cov["mod_double-top"] += 1
    if top or big_ge(d, n):
        return big_sub(d, n)[0]
    return d


_CONST = {}


def wave_constants(n, cov):
    """rsa_wave's per-key derivation: ninv by Newton, R mod n = 2^bits - n and (container - bits) doublings, 2R, then
    log2(container) Montgomery squarings -> R^2 mod n.  (The key cache keeps these; the model keeps them per modulus.)"""
    if n in _CONST:
        return _CONST[n]
    bits = n.bit_length()
    NL = 1 if bits <= 2048 else 2
    C = 2048 * NL
    nn = limbs(n, NL)
    n0 = n & M32
    x = n0
    for _ in range(5):
        x = x * (2 - n0 * x) & M32
    ninv = -x & M32
    assert ninv * n0 & M32 == M32                                  # -n^-1 mod 2^32
    pw = limbs(1 << bits if bits < C else 0, NL)
    one = big_sub(pw, nn)[0]
    for _ in range(bits, C):
        one = mod_double(one, nn, cov)
    if bits < C:
        cov["mod_double-R", NL] += 1
    assert value(one) == (1 << C) % n
    rr = mod_double(one, nn, cov)
    for _ in range(11 if NL == 1 else 12):
        rr = mont_mul(rr, rr, nn, ninv, cov)
    assert value(rr) == pow(2, 2 * C, n)
    _CONST[n] = (nn, ninv, rr)
    return _CONST[n]


def wave_modexp(s, e, n, cov):
    """rsa_wave's arithmetic for s < n: s R, left-to-right square-and-multiply in the Montgomery domain, times 1 out of it"""
    nn, ninv, rr = wave_constants(n, cov)
    NL = len(nn) // 64
    xm = mont_mul(limbs(s, NL), rr, nn, ninv, cov)
    acc = xm
    e = e | (e == 0)
    for bit in reversed(range(e.bit_length() - 1)):
        acc = mont_mul(acc, acc, nn, ninv, cov)
        if (e >> bit) & 1:
            acc = mont_mul(acc, xm, nn, ninv, cov)
    return value(mont_mul(acc, limbs(1, NL), nn, ninv, cov))


# ---- the wave routine ------------------------------------------------------------------------------------------------

def _wave_subset():
    """the accepted cases of rc.wave_cases() whose exponent is 65537 (it rotates the exponents over the signatures), and
    every exponent of the list on n - 1 and the c0 values of a few moduli"""
    picked = []
    for n, e, s, tag in rc.wave_cases():
        if s >= n or n.bit_length() < 2:
            continue
        mt, st = tag.split("/")[:2]
        if e == 65537 or (st in ("n-1", "c0") and mt in ("2^2048-c", "2^4096-c", "edge2049", "edge1025", "tiny3", "mersenne61")):
            picked.append((n, e, s, tag))
    return picked


@pytest.fixture(scope="module")
def wave_run():
    cov = Counter()
    cases = _wave_subset()
    for n, e, s, tag in cases:
        assert wave_modexp(s, e, n, cov) == pow(s, e, n), tag
    return cases, cov


def test_wave_model_matches_pow(wave_run):
    cases, _ = wave_run
    assert len(cases) >= 200
    assert {e for _, e, _, _ in cases} == set(rc.WAVE_EXPONENTS)
    assert {n.bit_length() for n, _, _, _ in cases} >= {2, 61, 512, 1024, 2047, 2048, 2049, 3072, 4095, 4096}


def test_wave_edge_cases_reach_the_carry_paths(wave_run):
    """c0 (one and two limbs per lane), a carry out of the lane-63 hand-off, the overflow word of big_normalize (top != 0),
    mod_double on moduli short of their container; and c0 comes from the 'c0' signatures, not from random operands.
    mod_double's own overflow bit is unreachable: it doubles R - n < 2^(C-1) (a modulus of C bits) or values below a
    modulus of fewer than C bits, so bit C - 1 of its operand is never set."""
    cases, cov = wave_run
    assert cov["c0", 1] > 0 and cov["c0", 2] > 0, cov
    assert cov["handoff"] > 0 and cov["normalize-crosses-groups"] > 0, cov
    assert cov["top", 1] > 0 and cov["top", 2] > 0, cov
    assert cov["mod_double-R", 1] > 0 and cov["mod_double-R", 2] > 0, cov
    assert cov["mod_double-top"] == 0, cov
    c0_only = Counter()
    for n, e, s, tag in cases:
        if "/c0/" in tag and e == 65537:
            wave_modexp(s, e, n, c0_only)
    assert c0_only["c0", 1] > 0 and c0_only["c0", 2] > 0, c0_only
    rng = random.Random(3)
    for k in (2048, 4096):                                           # a random modulus and signature: no c0 in a whole chain
        n = rc.rand_odd(k, rng)
        c = Counter()
        s = rng.randrange(n)
        assert wave_modexp(s, 65537, n, c) == pow(s, 65537, n)
        assert c["c0", k // 2048] == 0, c


# ---- the lane-group routine -----------------------------------------------------------------------------------------

def group_check(s, n, G):
    """rsa_group_wave's s >= n check: per lane the sign of the highest differing limb, the highest differing lane of the
    group decides.  -> (reject, deciding lane or None)"""
    sl, nl = gm.to_lanes(s, G), gm.to_lanes(n, G)
    c = []
    for p in range(G):
        d = 0
        for j in reversed(range(gm.QL)):
            d = d or (sl[p][j] > nl[p][j]) - (sl[p][j] < nl[p][j])
        c.append(d)
    gt = sum(1 << p for p in range(G) if c[p] > 0)
    lt = sum(1 << p for p in range(G) if c[p] < 0)
    return gt >= lt, ((gt | lt).bit_length() - 1 if gt | lt else None)


def group_before_sub(s, n, G):
    """group_modexp up to its last step: the exact-limb value the final conditional subtraction gets"""
    Rbits = 28 * gm.QL * G
    rr = gm.to_lanes(pow(2, 2 * Rbits, n), G)
    ninv = (-pow(n, -1, 1 << 28)) & gm.MASK
    nn = gm.to_lanes(n, G)
    acc = plain = gm.to_lanes(s, G)
    for step in range(18):
        b = rr if step == 0 else (plain if step == 17 else acc)
        acc = gm.qnorm(gm.qmont_columns(acc, b, nn, ninv, G), G, G - 1 if step == 17 else 1)
    return acc, nn


def sub_borrows(acc, nn, G):
    """cond_sub's decision: None when acc < n, else the set of lanes that start the subtraction with a borrow"""
    taken, _ = group_check(gm.from_lanes(acc), gm.from_lanes(nn), G)
    if not taken:
        return None
    a, n = gm.from_lanes(acc), gm.from_lanes(nn)
    return {p for p in range(1, G) if a % (1 << (rc.LANE_BITS * p)) < n % (1 << (rc.LANE_BITS * p))}


@pytest.mark.parametrize("G", [4, 8])
def test_group_check_decided_by_every_lane(G):
    """n -+ 2^(532 p): lane p is the highest lane of the group where s and n differ; the check must reject s >= n and
    accept s < n whichever lane decides."""
    rng = random.Random(G)
    keys = synth.load_keys()
    seen = Counter()
    mods = [n for _, n in rc.moduli() if rc.group_lanes(n.bit_length()) == G] + \
           [k.n for k in keys.values() if k.n.bit_length() >= 512 and rc.group_lanes(k.n.bit_length()) == G]
    for n in mods:
        for s, tag in rc.signatures(n, rng, G):
            reject, lane = group_check(s, n, G)
            assert reject == (s >= n), (hex(n)[:16], tag)
            if lane is not None and (tag.startswith("n-lane") or tag.startswith("reject-lane")):
                seen[reject, lane] += 1
    for p in range(G):
        assert seen[True, p] > 0 and seen[False, p] > 0, (p, seen)


@pytest.mark.parametrize("G,name", [(4, "rsa2048_03"), (4, "rsa2047_00"), (8, "rsa4096_03"), (8, "rsa4095_00")])
def test_group_final_subtraction_borrows_into_every_lane(G, name):
    """s = t^d mod n with t 200-300 bits short of n: the last product leaves t + n, the final subtraction runs, and the
    lanes it starts with a borrow cover 1..G-1 (t = 2^m - 1 carries out of every lane boundary below m)."""
    k = synth.load_keys()[name]
    rng = random.Random(k.n & 0xFFFF)
    lanes = set()
    for s, tag in rc.small_result_signatures(k, rng):
        acc, nn = group_before_sub(s, k.n, G)
        b = sub_borrows(acc, nn, G)
        assert b is not None, tag                                    # the subtraction is taken
        lanes |= b
        assert gm.from_lanes(gm.cond_sub(acc, nn, G)) == pow(s, 65537, k.n), tag
    assert lanes == set(range(1, G)), lanes
    for s, tag in rc.signatures(k.n, rng, G, with_rejects=False)[:3]:       # 0, 1, 2: never
        acc, nn = group_before_sub(s, k.n, G)
        assert sub_borrows(acc, nn, G) is None, tag


def test_group_final_subtraction_unreachable_for_1024_bits():
    """Four lanes on a 1024-bit key: R = 2^2128 > n^2 2^80, so the last product's excess n s^65536 R / R ... is below
    n^2 / R < 1 ulp of n: acc = t exactly and the subtraction is never taken, not even for small t."""
    k = synth.load_keys()["rsa1024_00"]
    rng = random.Random(1)
    for s, tag in rc.small_result_signatures(k, rng):
        acc, nn = group_before_sub(s, k.n, 4)
        assert sub_borrows(acc, nn, 4) is None and gm.from_lanes(acc) == pow(s, 65537, k.n), tag
