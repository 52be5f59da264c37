"""CPU (-m "not gpu"): a Python-integer model of csrc/rsa_quad.hip.h as it is NOW — G lanes per signature, QL = 18 limbs
of QBITS = 29 bits per lane, a window of 36 64-bit columns per lane, quotient digits from lane 0, the low half of a window
handed one lane down every 18 steps, no conditional subtraction until the very end — step for step as the kernel does it,
with the kernel's register widths asserted (every accumulator < 2^64, every operand limb <= 2^29, the local carry of the
normalisation < 2^35, 32-bit sums in its cross-lane passes).

tests/test_rsa_group_model.py is the same model at 19 limbs of 28 bits, the layout the routine had before; it is
self-contained and keeps passing, but THIS file describes the code (rsa.hip.h: QL, QBITS; KeyCacheEntry::rrq).

Results must equal pow(s, 65537, n) for random and worst-case operands, four lanes (<= 2048 bits) and eight (<= 4096);
the cached constant must be what the pre-pass of rsa_kernel.hip.h derives from 2^(2 * 2048 NL) mod n with two
32-bit-radix Montgomery products and c = 80 / 160; values that straddle a lane boundary (522 bits per lane) go through
the s >= n check, the arithmetic and the final subtraction."""
import random

import pytest

QL, QBITS = 18, 29
MASK = (1 << QBITS) - 1
LANE_BITS = QL * QBITS                                                # 522
U64 = 1 << 64


def to_lanes(x, G):
    assert x < 1 << (LANE_BITS * G)
    limbs = [(x >> (QBITS * t)) & MASK for t in range(G * QL)]
    return [limbs[QL * p:QL * (p + 1)] for p in range(G)]


def from_lanes(v):
    return sum(l << (QBITS * (QL * p + j)) for p, lane in enumerate(v) for j, l in enumerate(lane))


def qmont_columns(a, b, n, ninv, G, stats=None):
    """qmont_columns<G>: returns W[p][0 .. 2 QL) of which [0, QL) are the lazy columns of the result."""
    assert all(l <= MASK + 1 for x in (a, b) for lane in x for l in lane)       # operand limbs <= 2^29
    assert all(l <= MASK for lane in n for l in lane)
    W = [[0] * (2 * QL) for _ in range(G)]
    B = [list(x) for x in b]
    for _blk in range(G):
        for r in range(QL):
            bd = B[0][r]                                             # g_bcast0
            for p in range(G):
                for k in range(QL):
                    base = 0 if (k == QL - 1 and r > 0) else W[p][k + r]      # first touch of a high column
                    W[p][k + r] = a[p][k] * bd + base
                    assert W[p][k + r] < U64
            m = ((W[0][r] & 0xFFFFFFFF) * ninv) & MASK                # lane 0's quotient digit, broadcast
            for p in range(G):
                for k in range(QL):
                    W[p][k + r] = n[p][k] * m + W[p][k + r]
                    assert W[p][k + r] < U64
                carry = W[p][r] >> QBITS
                assert carry < 1 << 35
                W[p][r + 1] += carry
                assert W[p][r + 1] < U64
                if stats is not None:
                    stats["peak"] = max(stats.get("peak", 0), W[p][r], W[p][r + 1])
                W[p][r] &= MASK
            assert W[0][r] == 0                                      # reduced
        recv = [[W[(p + 1) % G][j] for j in range(QL)] for p in range(G)]      # g_rotdown of the finished low columns
        for p in range(G):
            for j in range(QL):
                assert recv[p][j] <= MASK                            # the kernel moves 32 bits of the column
                W[p][j] = W[p][QL + j] + recv[p][j]
                assert W[p][j] < U64
        B = [B[(p + 1) % G] for p in range(G)]                       # g_rotdown of the multiplier digits
    return W


def qnorm(W, G, cross):
    out = [[0] * QL for _ in range(G)]
    carry = [0] * G
    for p in range(G):
        c = 0
        for j in range(QL):
            t = W[p][j] + c
            assert t < U64
            out[p][j] = t & MASK
            c = t >> QBITS
        assert c < 1 << 35                                           # clo / chi of the kernel
        carry[p] = c
    for npass in range(cross):
        cin = [0] + carry[:-1]                                       # g_fromprev, lane 0 masked
        for p in range(G):
            t = out[p][0] + cin[p]
            out[p][0] = t & MASK
            c = t >> QBITS
            assert c < (1 << 7 if npass == 0 else 2)
            for j in range(1, QL):
                t = out[p][j] + c
                assert t < (1 << 32)
                out[p][j] = t & MASK
                c = t >> QBITS
            carry[p] = c
    assert carry[G - 1] == 0                                         # nothing beyond 522 G bits
    last = [0] + carry[:-1]
    for p in range(G):
        assert last[p] <= 1
        out[p][0] += last[p]
        assert out[p][0] <= MASK + 1
    return out


def lane_compare(x, nn, G):
    """Per lane the sign of the highest differing limb -> the group's (gt, lt) masks; x >= n  <=>  gt >= lt."""
    gt = lt = 0
    for p in range(G):
        d = 0
        for j in reversed(range(QL)):
            if d == 0:
                d = (x[p][j] > nn[p][j]) - (x[p][j] < nn[p][j])
        gt |= (d > 0) << p
        lt |= (d < 0) << p
    return gt, lt


def cond_sub(acc, nn, G):
    """The last step of rsa_group_wave: acc (exact limbs, < 2n) minus n when acc >= n; the lanes below a lane decide the
    borrow it starts with."""
    gt, lt = lane_compare(acc, nn, G)
    if gt < lt:
        return acc
    out = []
    for p in range(G):
        low = (1 << p) - 1
        borrow = 1 if (lt & low) > (gt & low) else 0
        lane = []
        for j in range(QL):
            t = (acc[p][j] - nn[p][j] - borrow) & 0xFFFFFFFF           # 32-bit arithmetic: the borrow is bit 31
            lane.append(t & MASK)
            borrow = t >> 31
        out.append(lane)
    return out


def group_modexp(s, n, G, stats=None):
    """rsa_group_wave<G> for an accepted signature's arithmetic; s >= n runs with s = 0 as the kernel does."""
    Rbits = LANE_BITS * G
    assert (1 << Rbits) > 4 * n
    rr = to_lanes(pow(2, 2 * Rbits, n), G)
    ninv = (-pow(n, -1, 1 << 32)) & 0xFFFFFFFF & MASK                # the cached 32-bit value, masked at use
    assert (n * ninv + 1) & MASK == 0
    nn = to_lanes(n, G)
    plain = to_lanes(s, G)
    gt, lt = lane_compare(plain, nn, G)
    assert (gt >= lt) == (s >= n)
    if gt >= lt:
        plain = to_lanes(0, G)
    acc = plain
    # s R, sixteen squarings -> s^65536 R; the last product takes the PLAIN s: (s^65536 R) s / R = s^65537, out of the
    # Montgomery domain without a product by one
    for step in range(18):
        b = rr if step == 0 else (plain if step == 17 else acc)
        acc = qnorm(qmont_columns(acc, b, nn, ninv, G, stats), G, G - 1 if step == 17 else 1)
        assert from_lanes(acc) < 2 * n                               # no conditional subtraction: values stay below 2n
    assert all(l <= MASK for lane in acc for l in lane)              # exact limbs
    em = cond_sub(acc, nn, G)                                        # < n + n^2 / R: one subtraction at most
    return from_lanes(em)


def rand_odd(bits, rng):
    return rng.getrandbits(bits) | (1 << (bits - 1)) | 1


@pytest.mark.parametrize("G,bits", [(4, 1024), (4, 1537), (4, 2048), (8, 2049), (8, 3072), (8, 4096)])
def test_group_modexp_matches_pow(G, bits):
    rng = random.Random(2900 * G + bits)
    for trial in range(2):
        n = rand_odd(bits, rng)
        s = rng.randrange(n)
        assert group_modexp(s, n, G) == pow(s, 65537, n), (G, bits, trial)


@pytest.mark.parametrize("G,bits", [(4, 2048), (8, 4096)])
def test_group_modexp_worst_case_limbs(G, bits):
    """All-ones moduli: every limb of n and of s = n - 1 is 2^29 - 1, the largest products a column can be asked to hold.
    The peak column stays below 36 * 2^58 + the carries, as the header comment of rsa_quad.hip.h argues."""
    n = (1 << bits) - 1                                              # odd; not a product of two primes, irrelevant here
    stats = {}
    for s in (n - 1, n - 2, 0, 1, (1 << bits) - (1 << (bits - QBITS)) - 1):
        assert group_modexp(s, n, G, stats) == pow(s, 65537, n), (G, hex(s)[:20])
    assert stats["peak"] < 36 * (1 << 58) + 18 * (1 << 35) + (1 << 29) < U64
    n = (1 << (bits - 1)) + 1                                        # the smallest modulus of this length
    for s in (n - 1, n - 2, 0, 1):
        assert group_modexp(s, n, G) == pow(s, 65537, n)


@pytest.mark.parametrize("G,bits", [(4, 2048), (4, 1031), (8, 4096), (8, 2100)])
def test_conditional_subtraction(G, bits):
    """The kernel's last step on values a signature that verifies never produces (acc >= n): equal, one more, all borrows
    (n with zero low limbs), the largest value the last product can leave."""
    rng = random.Random(29 * G + bits)
    ns = [rand_odd(bits, rng), (1 << (bits - 1)) + 1, (1 << bits) - 1, (1 << (bits - 1)) + (1 << LANE_BITS) + 1,
          (1 << (bits - 1)) + (1 << (2 * LANE_BITS - 1)) + 1]           # zero low limbs: a borrow runs through whole lanes
    for n in ns:
        for x in (0, 1, n - 1, n, n + 1, n + (1 << LANE_BITS) - 1, n + (n >> 40), 2 * n - 1, rng.randrange(n), n + rng.randrange(n)):
            if x >= 1 << (LANE_BITS * G):
                continue
            got = from_lanes(cond_sub(to_lanes(x, G), to_lanes(n, G), G))
            assert got == (x - n if x >= n else x), (G, bits, hex(x)[:18])


@pytest.mark.parametrize("NL,G", [(1, 4), (2, 8)])
def test_cached_constant_derivation(NL, G):
    """rsa_kernel.hip.h: mont(R^2, 2^c) = 2^c R, mont(R^2, 2^c R) = 2^c R^2 (radix R = 2^(2048 NL), c = 80 / 160) must be
    R'^2 mod n for R' = 2^(522 G); 2^c is one bit of one 32-bit limb (limb c / 32, bit c % 32), and the 4 QL NL limbs of
    29 bits the pre-pass stores are the ones the lane groups read."""
    R = 1 << (2048 * NL)
    c = 2 * (LANE_BITS * G - 2048 * NL)
    assert c == (80 if NL == 1 else 160)
    assert (c >> 5, c & 31) == ((2, 16) if NL == 1 else (5, 0))
    rng = random.Random(29 + NL)
    for n in (rand_odd(2048 * NL - 5, rng), rand_odd(2048 * NL, rng), (1 << (2048 * NL)) - 1, rand_odd(1024 * NL + 1, rng)):
        Rinv = pow(R, -1, n)
        mont = lambda x, y: x * y * Rinv % n
        rr = R * R % n
        r2 = mont(rr, mont(rr, 1 << c))
        assert r2 == pow(2, 2 * LANE_BITS * G, n)
        stored = [(r2 >> (QBITS * t)) & MASK for t in range(4 * QL * NL)]
        assert sum(l << (QBITS * t) for t, l in enumerate(stored)) == r2           # 4 QL NL limbs hold every bit of a value < n
        assert [l for lane in to_lanes(r2, G) for l in lane] == stored


def lane_boundary_moduli(G, k):
    """[(p, n)]: n = 2^k - 2^(522 p) + 1 and n = 2^k - 2^(522 p) - 1, in turn, for the lane boundaries p below k (p >= 1: odd)"""
    return [(p, (1 << k) - (1 << (LANE_BITS * p)) + (1 if p & 1 else -1)) for p in range(1, G) if LANE_BITS * p < k - 1] + \
        [(1, (1 << k) - (1 << LANE_BITS) - 1)]


@pytest.mark.parametrize("G,bits", [(4, 2048), (8, 4096)])
def test_values_straddling_a_lane_boundary(G, bits):
    """x = 2^(522 p) +- 1 as signatures (limbs of 2^29 - 1 below a boundary next to zero limbs above it, or one bit above
    zeros), under moduli with the same shape — every boundary under the first modulus, a modulus' own boundary under the
    others; and n +- 2^(522 p): lane p alone decides s < n / s >= n."""
    for i, (pm, n) in enumerate(lane_boundary_moduli(G, bits)):
        assert n & 1 and n.bit_length() == bits
        for p in (range(G) if i == 0 else (pm,)):
            for x in ((1 << (LANE_BITS * p)) + 1, (1 << (LANE_BITS * p)) - 1):
                assert x < n
                assert group_modexp(x, n, G) == pow(x, 65537, n), (G, p, hex(x)[:12])
    rng = random.Random(G)
    n = rand_odd(bits, rng)
    for p in range(G):
        d = 1 << (LANE_BITS * p)
        if d < n:
            assert group_modexp(n - d, n, G) == pow(n - d, 65537, n)
            if n + d < 1 << (LANE_BITS * G):
                assert group_modexp(n + d, n, G) == 0                    # rejected: runs with s = 0
    assert group_modexp(n, n, G) == 0
