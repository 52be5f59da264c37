"""CPU (-m "not gpu"): a Python-integer model of rsa_quad.hip.h's <8, 9> instantiation — eight lanes per signature, nine limbs
of 29 bits per lane, the same 72 limbs and the same radix R = 2^2088 as four lanes of eighteen (tests/test_rsa_group_model29.py
models those) — written the way the kernel computes:

  * qmont_columns<8, 9>: a window of 18 columns per lane, every column a 64-bit register (asserted at every write);
  * the one-move rotations: at the hand-over the top lane receives NOTHING (the kernel masks whatever row_shl:1 brings it with a
    per-lane mask that is zero there; what the rotation would have brought is lane 0's finished column, zero by construction —
    asserted), and the top lane of the multiplier copy receives a value the model draws at random: it must never reach a digit
    broadcast;
  * the quotient digit masked between its two broadcast moves (same value as masked behind them);
  * qnorm<8, 9, 1> between products, qnorm<8, 9, 7> and the conditional subtraction at the end;
  * the EMSA check: limb classes over 72 limbs (lane p: limbs 9 p .. 9 p + 8) and the byte walk, eight lanes side by side.

Checked: the column bound at the worst-case operands, value < 2n after every product, exactness after the final subtraction, the
cached constant being the four-lane routine's, and the EMSA verdict against a byte-by-byte judge for every k."""
import random

import pytest

G, L, QBITS = 8, 9, 29
LIMBS = G * L                                                         # 72
MASK = (1 << QBITS) - 1
RBITS = QBITS * LIMBS                                                 # 2088
U64 = 1 << 64


def to_lanes(x):
    assert 0 <= x < 1 << RBITS
    limbs = [(x >> (QBITS * t)) & MASK for t in range(LIMBS)]
    return [limbs[L * p:L * (p + 1)] for p in range(G)]


def from_lanes(v):
    return sum(l << (QBITS * (L * p + j)) for p, lane in enumerate(v) for j, l in enumerate(lane))


def qmont_columns(a, b, n, ninv, rng, stats=None):
    assert all(l <= MASK + 1 for x in (a, b) for lane in x for l in lane)       # operand limbs <= 2^29 (qnorm<.., 1> leaves that)
    assert all(l <= MASK for lane in n for l in lane)
    W = [[0] * (2 * L) for _ in range(G)]
    B = [list(x) for x in b]
    fresh = [True] * G                                                # lane p of B still holds digits of b (not the junk the shift brings)
    for _blk in range(G):
        assert fresh[0]                                               # the digits broadcast in this block are b's
        for r in range(L):
            bd = B[0][r]
            for p in range(G):
                for k in range(L):
                    base = 0 if (k == L - 1 and r > 0) else W[p][k + r]
                    W[p][k + r] = a[p][k] * bd + base
                    assert W[p][k + r] < U64
            m = ((W[0][r] & 0xFFFFFFFF) * ninv) & 0xFFFFFFFF & MASK   # masked on the first broadcast move
            for p in range(G):
                for k in range(L):
                    W[p][k + r] = n[p][k] * m + W[p][k + r]
                    assert W[p][k + r] < U64
                carry = W[p][r] >> QBITS
                assert carry < 1 << 35
                W[p][r + 1] += carry
                assert W[p][r + 1] < U64
                if stats is not None:
                    stats["peak"] = max(stats.get("peak", 0), W[p][r], W[p][r + 1])
            assert W[0][r] & MASK == 0                                # lane 0's finished column: what a rotation would hand to the top lane
        for p in range(G):
            for j in range(L):
                recv = (W[p + 1][j] & 0xFFFFFFFF) & MASK if p < G - 1 else 0        # row_shl:1, masked; the top lane's mask is zero
                W[p][j] = W[p][L + j] + recv
                assert W[p][j] < U64
        B = [B[p + 1] if p < G - 1 else [rng.getrandbits(32) for _ in range(L)] for p in range(G)]
        fresh = fresh[1:] + [False]
    return W


def qnorm(W, cross):
    out = [[0] * L for _ in range(G)]
    carry = [0] * G
    for p in range(G):
        c = 0
        for j in range(L):
            t = W[p][j] + c
            assert t < U64
            out[p][j] = t & MASK
            c = t >> QBITS
        assert c < 1 << 35
        carry[p] = c
    for npass in range(cross):
        cin = [0] + carry[:-1]
        for p in range(G):
            t = out[p][0] + cin[p]
            out[p][0] = t & MASK
            c = t >> QBITS
            assert c < (1 << 7 if npass == 0 else 2)
            for j in range(1, L):
                t = out[p][j] + c
                assert t < 1 << 32
                out[p][j] = t & MASK
                c = t >> QBITS
            carry[p] = c
    assert carry[G - 1] == 0
    last = [0] + carry[:-1]
    for p in range(G):
        assert last[p] <= 1
        out[p][0] += last[p]
        assert out[p][0] <= MASK + 1
    return out


def lane_compare(x, nn):
    gt = lt = 0
    for p in range(G):
        d = 0
        for j in reversed(range(L)):
            if d == 0:
                d = (x[p][j] > nn[p][j]) - (x[p][j] < nn[p][j])
        gt |= (d > 0) << p
        lt |= (d < 0) << p
    return gt, lt


def cond_sub(acc, nn):
    gt, lt = lane_compare(acc, nn)
    if gt < lt:
        return acc
    out = []
    for p in range(G):
        low = (1 << p) - 1
        borrow = 1 if (lt & low) > (gt & low) else 0
        lane = []
        for j in range(L):
            t = (acc[p][j] - nn[p][j] - borrow) & 0xFFFFFFFF
            lane.append(t & MASK)
            borrow = t >> 31
        out.append(lane)
    return out


def ninv_of(n):
    return (-pow(n, -1, 1 << 32)) & 0xFFFFFFFF & MASK


def group_modexp(s, n, rng, stats=None):
    assert (1 << RBITS) > 4 * n
    rr = to_lanes(pow(2, 2 * RBITS, n))
    nn, plain = to_lanes(n), to_lanes(s)
    gt, lt = lane_compare(plain, nn)
    assert (gt >= lt) == (s >= n)
    if gt >= lt:
        plain = to_lanes(0)
    acc = plain
    for step in range(18):
        b = rr if step == 0 else (plain if step == 17 else acc)
        acc = qnorm(qmont_columns(acc, b, nn, ninv_of(n), rng, stats), G - 1 if step == 17 else 1)
        assert from_lanes(acc) < 2 * n                               # value < 2n after every product
    assert all(l <= MASK for lane in acc for l in lane)
    return from_lanes(cond_sub(acc, nn))


def rand_odd(bits, rng):
    return rng.getrandbits(bits) | (1 << (bits - 1)) | 1


@pytest.mark.parametrize("bits", [512, 1024, 1537, 2047, 2048])
def test_modexp_matches_pow(bits):
    rng = random.Random(900 + bits)
    for trial in range(2):
        n = rand_odd(bits, rng)
        for s in (rng.randrange(n), 0, 1, n - 1):
            assert group_modexp(s, n, rng) == pow(s, 65537, n), (bits, trial)
        assert group_modexp(n, n, rng) == 0 and group_modexp(n + 2, n, rng) == 0          # rejected: runs with s = 0


def test_column_bound_at_the_worst_case_operands():
    """A column lives through 2 L = 18 products of at most 2^29 * 2^29 (operand limbs may be 2^29 itself out of qnorm<.., 1>),
    two carries below 2^35 and one received limb: the bound the header states.  Driven at it: a product of two operands whose
    every limb is 2^29 - 1 under n = 2^2048 - 1 (every limb of n that exists is all ones), and whole exponentiations under that
    modulus and under moduli just above 2^2047."""
    rng = random.Random(99)
    bound = 18 * (1 << 58) + 2 * (1 << 35) + (1 << 29)
    assert bound < U64 // 2                                           # "more room, not less": 2^62.2; the 18-limb layout sits at 2^63.2
    n = (1 << 2048) - 1
    ones = [[MASK] * L for _ in range(G)]
    stats = {}
    qmont_columns(ones, ones, to_lanes(n), ninv_of(n), rng, stats)           # (operands of 2^2088 - 1 are far above 2n: only the columns count here)
    assert stats["peak"] > L * MASK * MASK                            # the a * b half of a column at its maximum (the quotient digits are what they are)
    for s in (n - 1, n - 2, 0, 1, (1 << 2048) - (1 << (2048 - QBITS)) - 1):
        assert group_modexp(s, n, rng, stats) == pow(s, 65537, n)
    for n in ((1 << 2047) + 1, (1 << 2047) + (1 << (QBITS * L)) + 1, (1 << 2047) + (1 << 2046) - 1 | 1):
        assert n.bit_length() == 2048 and n & 1
        for s in (n - 1, n - 2, 0, 1, rng.randrange(n)):
            assert group_modexp(s, n, rng, stats) == pow(s, 65537, n)
    assert stats["peak"] < bound


def test_final_subtraction_is_exact():
    """acc >= n never happens for a signature that verifies; the step is driven here on its own: equal, one more, borrows that
    run through whole lanes (n with zero low limbs), the largest value the last product can leave (< n + n^2 / R)."""
    rng = random.Random(7)
    lane = 1 << (QBITS * L)
    for bits in (2048, 2047, 1031, 512):
        ns = [rand_odd(bits, rng), (1 << (bits - 1)) + 1, (1 << bits) - 1]
        ns += [(1 << (bits - 1)) + (lane << (QBITS * L * q)) + 1 for q in range(3) if QBITS * L * (q + 1) < bits - 1]
        for n in ns:
            for x in (0, 1, n - 1, n, n + 1, n + lane - 1, n + (n >> 40), 2 * n - 1, rng.randrange(n), n + rng.randrange(n)):
                got = from_lanes(cond_sub(to_lanes(x), to_lanes(n)))
                assert got == (x - n if x >= n else x), (bits, hex(x)[:18])


def test_cached_constant_is_the_four_lane_one():
    """KeyCacheEntry::rrq holds R'^2 mod n for R' = 2^(29 * 18 * 4) as limbs t = 0 .. 71; lane p of four reads limbs 18 p + j, lane
    p of eight reads limbs 9 p + j: the same 72 words, because 8 * 9 = 4 * 18 is the same radix."""
    assert RBITS == 29 * 18 * 4
    rng = random.Random(3)
    n = rand_odd(2048, rng)
    r2 = pow(2, 2 * RBITS, n)
    stored = [(r2 >> (QBITS * t)) & MASK for t in range(4 * 18)]
    assert [l for lane in to_lanes(r2) for l in lane] == stored


# ---- the EMSA check on limbs -------------------------------------------------------------------------------------------
SHA256_DI = bytes.fromhex("3031300d060960864801650304020105000420")
SHA1_DI = bytes.fromhex("3021300906052b0e03021a05000414")
EM_BYTES = 256


def emsa_ok_bytes(em_le, k, sha1):
    """the byte-by-byte judge: little-endian EM (index 0 = last byte), any digest"""
    di, hl = (SHA1_DI, 20) if sha1 else (SHA256_DI, 32)
    tlen = len(di) + hl
    if k < tlen + 11:
        return False
    want = bytes([0, 1]) + b"\xff" * (k - tlen - 3) + b"\0" + di
    be = bytes(reversed(em_le[:k]))
    return be[:k - hl] == want and not any(em_le[k:])


def emsa_ok_limbs(em, k, sha1):
    """rsa_group_wave<8, 9>: limb compares in lane p = t / 9, then the two stretches of the byte walk, lanes side by side"""
    di, hl = (SHA1_DI, 20) if sha1 else (SHA256_DI, 32)
    tlen = len(di) + hl
    limbs = [(em >> (QBITS * t)) & MASK for t in range(LIMBS)] + [0] * 4
    ff_lo, ff_hi = (8 * (tlen + 1) + QBITS - 1) // QBITS, (8 * (k - 2)) // QBITS
    z_lo = (8 * k + QBITS - 1) // QBITS
    bad = False
    for p in range(G):
        for j in range(L):
            t = L * p + j
            if ff_lo <= t < ff_hi:
                bad = bad or limbs[t] != MASK
            elif t >= z_lo:
                bad = bad or limbs[t] != 0
    walk_lo, walk_hi = (QBITS * ff_lo + 7) // 8, (QBITS * ff_hi) // 8
    walk_end = min((QBITS * z_lo + 7) // 8, EM_BYTES)

    def want_byte(i):                                                 # emsa_byte for i >= hl
        if i >= k:
            return 0
        if i < tlen:
            return di[len(di) - 1 - (i - hl)]
        if i == tlen:
            return 0
        return 0xFF if i < k - 2 else (1 if i == k - 2 else 0)
    walked = set()
    for lo, hi in ((0, walk_lo), (walk_hi, walk_end)):
        for p in range(G):
            for i in range(lo + p, hi, G):
                t = (8 * i) // QBITS
                assert t + 1 < LIMBS + 4
                got = ((limbs[t] | (limbs[t + 1] << QBITS)) >> (8 * i - QBITS * t)) & 0xFF
                walked.add(i)
                if i >= hl:
                    bad = bad or got != want_byte(i)
    return (not bad) and k >= tlen + 11, walked


@pytest.mark.parametrize("sha1", [False, True])
def test_emsa_limb_classes_for_every_k(sha1):
    """For every modulus length k the routine can meet (64 .. 256 bytes; below tLen + 11 refused outright): a well-formed EM
    passes, and a flip of any single byte outside the digest — FF run, 01, top 00, separator, DigestInfo, and every byte at or
    above k up to the 256 the limbs cover — fails, exactly as the byte-by-byte judge says.  A byte the walk skips must lie
    wholly inside limbs of one class."""
    rng = random.Random(5 + sha1)
    di, hl = (SHA1_DI, 20) if sha1 else (SHA256_DI, 32)
    tlen = len(di) + hl
    for k in list(range(40, 80)) + list(range(80, 250, 13)) + [127, 128, 129, 191, 192, 247, 248, 249, 250, 251, 252, 253, 254, 255, 256]:
        digest = bytes(rng.getrandbits(8) for _ in range(hl))
        if k < tlen + 11:
            em = int.from_bytes(b"\0\1" + b"\xff" * max(0, k - tlen - 3) + b"\0" + di + digest, "big") & ((1 << (8 * k)) - 1)
            assert emsa_ok_limbs(em, k, sha1)[0] is False
            continue
        be = b"\0\1" + b"\xff" * (k - tlen - 3) + b"\0" + di + digest
        em = int.from_bytes(be, "big")
        ok, walked = emsa_ok_limbs(em, k, sha1)
        assert ok and emsa_ok_bytes(em.to_bytes(EM_BYTES, "little"), k, sha1), k
        for i in range(hl, EM_BYTES):
            for flip in (0x01, 0x80, 0xFF):
                bad_em = em ^ (flip << (8 * i))
                got = emsa_ok_limbs(bad_em, k, sha1)[0]
                assert got == emsa_ok_bytes(bad_em.to_bytes(EM_BYTES, "little"), k, sha1) and not got, (k, i, flip)
        assert set(range(hl)) <= walked                               # the digest bytes are all handed over
        # a short FF run, 00 where FF belongs, and the run one byte longer (separator overwritten)
        for pos in (tlen + 1, (tlen + k) // 2, k - 3):
            assert not emsa_ok_limbs(em & ~(0xFF << (8 * pos)), k, sha1)[0], (k, pos)
        assert not emsa_ok_limbs(em | (0xFF << (8 * tlen)), k, sha1)[0]
