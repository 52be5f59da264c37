"""CPU (-m "not gpu"): Python-integer models of the two things csrc/rsa_quad.hip.h does differently from the model in
tests/test_rsa_group_model29.py, which stays the description of the arithmetic:

(a) qmont_columns with the masks deferred:
      * the quotient digit is masked to 29 bits AFTER its broadcast (the broadcast moves the 32-bit product);
      * a finished column is NOT masked inside the step; the lane that receives it at the hand-over masks the 32 bits it gets;
      * the digit of step r of block blk, lane 0 of the rotating multiplier copy, is b[blk][r]: reading it from lane blk of the
        operand directly (the written-out variant that was measured and not kept) is the same value.
    Every column must stay below 2^64 — the unmasked column is only ever read through its low 32 bits and its carry, so the
    bound of the header comment is unchanged — and every value the next stage reads must equal the model29 routine's.

(b) the EMSA-PKCS1-v1_5 shape check on limbs: a limb whose 29 bits lie wholly in the FF run must equal 2^29 - 1, a limb wholly
    at or above bit 8k must be 0, and the byte walk visits only the bytes of the remaining (boundary) limbs, with emsa_byte as
    the judge of each.  The classification is checked bit by bit against emsa_byte for every k, and the verdict against the
    full byte walk for every single-bit corruption of a well-formed EM."""
import random

import pytest

import test_rsa_group_model29 as m29
from test_rsa_group_model29 import LANE_BITS, MASK, QBITS, QL, U64, from_lanes, rand_odd, to_lanes

M32 = 0xFFFFFFFF


# ---- (a) the product with deferred masks ------------------------------------------------------------------------------

def qmont_columns_trim(a, b, n, ninv, G, stats=None):
    """qmont_columns<G> as rsa_quad.hip.h has it: W[p][0 .. QL) are the lazy columns of the result."""
    assert all(l <= MASK + 1 for x in (a, b) for lane in x for l in lane)       # operand limbs <= 2^29
    assert all(l <= MASK for lane in n for l in lane)
    W = [[0] * (2 * QL) for _ in range(G)]
    B = [list(x) for x in b]                                         # the rotating copy
    for blk in range(G):
        for r in range(QL):
            bd = B[0][r]                                             # g_bcast0 of the rotated copy
            assert bd == b[blk][r]                                   # = lane blk of the operand
            for p in range(G):
                for k in range(QL):
                    base = 0 if (k == QL - 1 and r > 0) else W[p][k + r]
                    W[p][k + r] = a[p][k] * bd + base
                    assert W[p][k + r] < U64
            m = (((W[0][r] & M32) * ninv) & M32) & MASK              # lane 0's 32-bit product is broadcast, every lane masks it
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
                # (no mask here: column r is read again only at the hand-over, through its low 32 bits)
            assert W[0][r] & MASK == 0                               # reduced: lane 0 hands a zero up to the top lane
        recv = [[(W[(p + 1) % G][j] & M32) & MASK for j in range(QL)] for p in range(G)]      # masked where it is received
        for p in range(G):
            for j in range(QL):
                W[p][j] = W[p][QL + j] + recv[p][j]
                assert W[p][j] < U64
        B = [B[(p + 1) % G] for p in range(G)]
    return W


def ninv_of(n):
    return (-pow(n, -1, 1 << 32)) & M32 & MASK


def check_product(a, b, n, G, stats=None, beside=True):
    """one product: a b / R mod n within [0, 2n), and (beside) the same columns as model29's routine gives"""
    R = 1 << (LANE_BITS * G)
    al, bl, nl = to_lanes(a, G), to_lanes(b, G), to_lanes(n, G)
    W = qmont_columns_trim(al, bl, nl, ninv_of(n), G, stats)
    if beside:
        ref = m29.qmont_columns(al, bl, nl, ninv_of(n), G)
        assert [w[:QL] for w in W] == [w[:QL] for w in ref]
    got = from_lanes(m29.qnorm(W, G, G - 1))
    assert got < 2 * n and got % n == a * b * pow(R, -1, n) % n
    return got


def group_modexp_trim(s, n, G, stats=None):
    """m29.group_modexp over the trimmed product (s < n)"""
    Rbits = LANE_BITS * G
    rr, nn, plain = to_lanes(pow(2, 2 * Rbits, n), G), to_lanes(n, G), to_lanes(s, G)
    acc = plain
    for step in range(18):
        b = rr if step == 0 else (plain if step == 17 else acc)
        acc = m29.qnorm(qmont_columns_trim(acc, b, nn, ninv_of(n), G, stats), G, G - 1 if step == 17 else 1)
        assert from_lanes(acc) < 2 * n
    return from_lanes(m29.cond_sub(acc, nn, G))


def alternating(bits, first):
    x = sum(MASK << (QBITS * t) for t in range(first ^ 1, bits // QBITS + 2, 2))
    return x & ((1 << bits) - 1)


def edge_operands(n, G):
    """all-ones limbs, alternating limbs, n - 1, values on both sides of every lane boundary (model29's edge operands)"""
    bits = n.bit_length()
    out = [0, 1, n - 1, n - 2, (1 << (bits - 1)) - 1, alternating(bits - 1, 1), alternating(bits - 1, 0)]
    for p in range(1, G):
        d = 1 << (LANE_BITS * p)
        if d + 1 < n:
            out += [d - 1, d, d + 1, n - d]
    return [x for x in out if 0 <= x < n]


@pytest.mark.parametrize("G,bits", [(4, 1024), (4, 1537), (4, 2048), (8, 2049), (8, 3072), (8, 4096)])
def test_product_random_operands(G, bits):
    rng = random.Random(31 * G + bits)
    for _ in range(3):
        n = rand_odd(bits, rng)
        # operands as the loop feeds them: anything below 2n (lazy values), and a plain value below n
        check_product(rng.randrange(2 * n), rng.randrange(2 * n), n, G)
        check_product(rng.randrange(2 * n), rng.randrange(n), n, G)


@pytest.mark.parametrize("G,bits", [(4, 2048), (8, 4096)])
def test_product_edge_operands(G, bits):
    """Edge operands in a ring (each times itself and times its neighbour) under a random modulus; a shorter ring under the
    all-ones modulus (the largest products a column can hold), the smallest modulus of the length and two lane-boundary moduli.
    The peak column obeys the header comment's bound."""
    rng = random.Random(G)
    stats = {}
    boundary = [n for _, n in m29.lane_boundary_moduli(G, bits)]
    moduli = [rand_odd(bits, rng), (1 << bits) - 1, (1 << (bits - 1)) + 1, boundary[0], boundary[-1]]
    for i, n in enumerate(moduli):
        ops = edge_operands(n, G)
        if i > 0:
            ops = ops[2:7] + ops[-2:]
        for j, x in enumerate(ops):
            check_product(x, ops[(j + 1) % len(ops)], n, G, stats, beside=i == 0)
            if i < 2:
                check_product(x, x, n, G, stats, beside=False)
    assert stats["peak"] < 36 * (1 << 58) + 18 * (1 << 35) + (1 << 29) < U64


@pytest.mark.parametrize("G,bits", [(4, 1024), (4, 2048), (8, 2049), (8, 4096)])
def test_modexp_matches_pow(G, bits):
    rng = random.Random(17 * G + bits)
    n = rand_odd(bits, rng) if bits % 1024 else (1 << bits) - 1       # the full sizes: all-ones limbs throughout
    s = rng.randrange(n) if bits % 1024 else n - 1
    stats = {}
    assert group_modexp_trim(s, n, G, stats) == pow(s, 65537, n)
    assert stats["peak"] < 36 * (1 << 58) + 18 * (1 << 35) + (1 << 29)


# ---- (b) the shape check on limbs -------------------------------------------------------------------------------------

SHA256_DIGESTINFO = bytes.fromhex("3031300d060960864801650304020105000420")
SHA1_DIGESTINFO = bytes.fromhex("3021300906052b0e03021a05000414")


def emsa_byte(q, k, digest, sha1):
    """rsa.hip.h emsa_byte: the EMSA-PKCS1-v1_5 byte at little-endian position q"""
    hl, pre = (20, SHA1_DIGESTINFO) if sha1 else (32, SHA256_DIGESTINFO)
    pl = len(pre)
    if q >= k:
        return 0
    if q < hl:
        return digest[hl - 1 - q]
    if q < hl + pl:
        return pre[pl - 1 - (q - hl)]
    if q == hl + pl or q == k - 1:
        return 0x00
    if q == k - 2:
        return 0x01
    return 0xFF


def limb_ranges(k, sha1, G):
    """rsa_group_wave's classifier: limbs [ff_lo, ff_hi) must be all ones, limbs >= z_lo zero; the walk visits bytes
    [0, walk_lo) and [walk_hi, walk_end).  (k >= tLen + 11, as the kernel requires before it believes the verdict.)"""
    tlen = 35 if sha1 else 51
    ff_lo = (8 * (tlen + 1) + QBITS - 1) // QBITS
    ff_hi = (8 * (k - 2)) // QBITS
    z_lo = (8 * k + QBITS - 1) // QBITS
    walk_lo = (QBITS * ff_lo + 7) // 8
    walk_hi = (QBITS * ff_hi) // 8
    walk_end = min((QBITS * z_lo + 7) // 8, 64 * G)
    return ff_lo, ff_hi, z_lo, walk_lo, walk_hi, walk_end


def limb_class(t, ff_lo, ff_hi, z_lo):
    return "ff" if ff_lo <= t < ff_hi else ("zero" if t >= z_lo else "walk")


def walked(i, walk_lo, walk_hi, walk_end):
    return i < walk_lo or walk_hi <= i < walk_end


def lanes_of(k):
    return 4 if k <= 256 else 8


@pytest.mark.parametrize("sha1", [False, True])
def test_classifier_agrees_with_emsa_byte_for_every_k(sha1):
    """Bit by bit, for every k of four lanes (62 .. 256; SHA-1 from 46) and of eight (257 .. 512).  Bits at or above 512 G
    lie outside the walk of either version: EM < n < 2^(8k) <= 2^(512 G) there."""
    digest = bytes(range(1, 33))
    hl = 20 if sha1 else 32
    for k in range(46 if sha1 else 62, 513):
        G = lanes_of(k)
        ff_lo, ff_hi, z_lo, walk_lo, walk_hi, walk_end = limb_ranges(k, sha1, G)
        assert ff_lo < ff_hi <= z_lo and walk_lo > hl            # the digest bytes (em_tail) are always walked
        for t in range(G * QL):
            c = limb_class(t, ff_lo, ff_hi, z_lo)
            for i in range(QBITS * t >> 3, (QBITS * t + QBITS - 1 >> 3) + 1):       # every byte that holds a bit of limb t
                if c == "ff":
                    assert emsa_byte(i, k, digest, sha1) == 0xFF and hl < i < k - 2, (k, t, i)
                elif c == "zero":
                    assert QBITS * t >= 8 * k and emsa_byte(i, k, digest, sha1) == 0, (k, t, i)
                elif i < 64 * G:
                    assert walked(i, walk_lo, walk_hi, walk_end), (k, t, i)
        # and the walk is short: the bottom tLen + 1 bytes and the limb straddling that edge, then at most three limbs on top
        n_walk = sum(1 for i in range(64 * G) if walked(i, walk_lo, walk_hi, walk_end))
        assert n_walk <= (51 + 1 + 4) + 3 * 4 + 1


def expected_image(k, sha1, G):
    """emsa_byte for every byte of the walk's 64 G (the digest bytes are not judged: zero here)"""
    hl = 20 if sha1 else 32
    return bytes(emsa_byte(i, k, bytes(hl), sha1) for i in range(64 * G))


def verdict_full(em, k, sha1, G, exp):
    """the byte walk over all 64 G bytes: (shape ok, digest bytes as em_tail gets them)"""
    hl = 20 if sha1 else 32
    b = em.to_bytes(LANE_BITS * G // 8 + 1, "little")
    return b[hl:64 * G] == exp[hl:], bytes(b[:hl])


def verdict_trim(em, k, sha1, G, exp):
    """limbs for the FF run and the zeros above k (the classes are the contiguous ranges the test above checks limb by limb),
    bytes for the rest"""
    hl = 20 if sha1 else 32
    ff_lo, ff_hi, z_lo, walk_lo, walk_hi, walk_end = limb_ranges(k, sha1, G)
    run = (1 << (QBITS * (ff_hi - ff_lo))) - 1
    ok = (em >> (QBITS * ff_lo)) & run == run                         # every limb of [ff_lo, ff_hi) equals 2^29 - 1
    ok = ok and (em >> (QBITS * z_lo)) & ((1 << (QBITS * (G * QL - z_lo))) - 1) == 0      # limbs z_lo .. G QL - 1 are zero
    b = em.to_bytes(LANE_BITS * G // 8 + 1, "little")
    ok = ok and b[hl:walk_lo] == exp[hl:walk_lo] and b[walk_hi:walk_end] == exp[walk_hi:walk_end]
    return ok, bytes(b[:hl])


@pytest.mark.parametrize("k", [128, 129, 255, 256, 257, 384, 512])
@pytest.mark.parametrize("sha1", [False, True])
def test_single_bit_corruptions_get_the_full_walks_verdict(k, sha1):
    """A well-formed EM and each of its 8k single-bit corruptions (exhaustive): the same verdict and the same digest bytes
    from the limb + boundary-walk check as from the full byte walk.  Only flips inside the digest keep the shape."""
    G = lanes_of(k)
    hl = 20 if sha1 else 32
    digest = bytes((37 * i + 11) & 0xFF for i in range(hl))
    em = int.from_bytes(bytes(emsa_byte(i, k, digest, sha1) for i in range(k)), "little")
    exp = expected_image(k, sha1, G)
    assert verdict_full(em, k, sha1, G, exp) == verdict_trim(em, k, sha1, G, exp) == (True, digest[::-1])
    for bit in range(8 * k):
        x = em ^ (1 << bit)
        full = verdict_full(x, k, sha1, G, exp)
        assert verdict_trim(x, k, sha1, G, exp) == full, (k, bit)
        assert full[0] == (bit < 8 * hl), (k, bit)
    # bits above 8k up to the end of the byte image (a value the arithmetic cannot produce under a k-byte modulus, but the
    # check must not depend on that)
    for bit in range(8 * k, 8 * 64 * G):
        x = em ^ (1 << bit)
        assert verdict_trim(x, k, sha1, G, exp) == verdict_full(x, k, sha1, G, exp) == (False, digest[::-1]), (k, bit)
