"""Ed25519 vectors shared by the oracle (CPU) and GPU tests: valid signatures from the Python-integer signer,
single-bit corruptions, and the edge cases that separate dalek's verify_strict from laxer rules.  Expectations
come from zkemail_rs_amd.ed25519_ref (Python ints), never from the oracle or the device."""
import numpy as np

import ed25519_ref as ed


def _enc(pt):
    return ed.compress(pt)


def torsion_points():
    """The eight points of order dividing 8, from a point of order 8 (RFC 8032 / dalek EIGHT_TORSION)."""
    # y of an order-8 point (well-known encoding c7176a70...); derive the group from it
    t8 = ed.decompress(bytes.fromhex("c7176a703d4dd84fba3c0b760d10670f2a2053fa2c39ccc64ec7fd7792ac037a"))
    assert t8 is not None and ed.is_identity(ed.mul(8, t8)) and not ed.is_identity(ed.mul(4, t8))
    return [ed.mul(i, t8) for i in range(8)]


def build_vectors(seed: int = 7, n_valid: int = 24):
    """-> list of (key32, msg32, sig64, expected) with expected in {0: key does not decode, 1: rejected, 2: valid}."""
    rng = np.random.default_rng(seed)
    out = []

    def rb(k):
        return rng.integers(0, 256, k, dtype=np.uint8).tobytes()

    def expect(key, msg, sig):
        if not ed.key_decodes(key):
            return 0
        return 2 if ed.verify_strict(key, msg, sig) else 1

    for _ in range(n_valid):
        sd, msg = rb(32), rb(32)
        pk, sig = ed.public_key(sd), ed.sign(sd, msg)
        out.append((pk, msg, sig, 2))
        # one flipped bit anywhere in R || S, in the message, in the key
        b = bytearray(sig); b[int(rng.integers(0, 64))] ^= 1 << int(rng.integers(0, 8))
        out.append((pk, msg, bytes(b), expect(pk, msg, bytes(b))))
        m = bytearray(msg); m[int(rng.integers(0, 32))] ^= 1 << int(rng.integers(0, 8))
        out.append((pk, bytes(m), sig, 1))
        k = bytearray(pk); k[int(rng.integers(0, 32))] ^= 1 << int(rng.integers(0, 8))
        out.append((bytes(k), msg, sig, expect(bytes(k), msg, sig)))
    # random byte strings as keys (about half are not curve points)
    for _ in range(32):
        k, msg, sig = rb(32), rb(32), rb(64)
        out.append((k, msg, sig, expect(k, msg, sig)))
    sd, msg = rb(32), rb(32)
    pk, sig = ed.public_key(sd), ed.sign(sd, msg)
    # S + L: same residue, non-canonical scalar -> rejected
    S = int.from_bytes(sig[32:], "little")
    out.append((pk, msg, sig[:32] + (S + ed.L).to_bytes(32, "little"), 1))
    # small-order A with the matching trivial signature (R = identity-ish, S = 0): lax verifiers accept, strict rejects
    for T in torsion_points():
        a = _enc(T)
        for Tr in torsion_points()[:3]:
            s0 = _enc(Tr) + (0).to_bytes(32, "little")
            out.append((a, msg, s0, expect(a, msg, s0)))
    # mixed-order A (valid point, not of small order): k is reduced mod L BEFORE the multiplication
    a_pt = ed.decompress(pk)
    for T in torsion_points()[1:4]:
        mixed = _enc(ed.add(a_pt, T))
        out.append((mixed, msg, sig, expect(mixed, msg, sig)))
    # small-order R on a good key
    for T in torsion_points()[:4]:
        s1 = _enc(T) + sig[32:]
        out.append((pk, msg, s1, expect(pk, msg, s1)))
    # non-canonical encodings: y >= p, and x = 0 with the sign bit set
    for y in (ed.P, ed.P + 1, ed.P + 3, ed.P + 4, ed.P + 18, 2 ** 255 - 1):
        for sgn in (0, 1):
            enc = (y | (sgn << 255)).to_bytes(32, "little")
            out.append((enc, msg, sig, expect(enc, msg, sig)))
            s2 = enc + sig[32:]
            out.append((pk, msg, s2, expect(pk, msg, s2)))
    for enc in ((1 | (1 << 255)).to_bytes(32, "little"), ((ed.P - 1) | (1 << 255)).to_bytes(32, "little")):
        out.append((enc, msg, sig, expect(enc, msg, sig)))
    return out


def build_edge_vectors(seed: int = 8):
    """-> list of (label, [(key, msg, sig, expected), ...]): one verify call per entry, equal-length messages within it.
    Message lengths 1..32, S at and around its boundaries, and the launch shapes of the 16-signatures-per-wave kernel:
    partial waves, waves whose other quads leave early, a wave that leaves as a whole, and the replicated tail."""
    rng = np.random.default_rng(seed)
    out = []

    def rb(k):
        return rng.integers(0, 256, k, dtype=np.uint8).tobytes()

    def expect(key, msg, sig):
        if not ed.key_decodes(key):
            return 0
        return 2 if ed.verify_strict(key, msg, sig) else 1

    def vec(key, msg, sig):
        return (key, msg, sig, expect(key, msg, sig))

    def with_s(sig, S):
        return sig[:32] + S.to_bytes(32, "little")

    # message length: a valid signature, and the same signature over a message with its last byte changed
    for ml in range(1, 33):
        sd, msg = rb(32), rb(ml)
        pk, sig = ed.public_key(sd), ed.sign(sd, msg)
        out.append(("msg_len %d" % ml, [vec(pk, msg, sig), vec(pk, msg[:-1] + bytes([msg[-1] ^ 0x40]), sig)]))
        assert [v[3] for v in out[-1][1]] == [2, 1]

    # S boundaries on an otherwise valid signature
    sd, msg = rb(32), rb(32)
    pk, sig = ed.public_key(sd), ed.sign(sd, msg)
    S = int.from_bytes(sig[32:], "little")
    wraps = [vec(pk, msg, with_s(sig, S + k * ed.L)) for k in range(1, (2 ** 256 - 1 - S) // ed.L + 1)]
    assert len(wraps) >= 14 and all(v[3] == 1 for v in wraps)
    out.append(("S + kL", wraps))
    out.append(("S boundaries", [vec(pk, msg, sig)] +
                [vec(pk, msg, with_s(sig, s)) for s in (ed.L - 1, ed.L, ed.L + 1, 0, 2 ** 252, 2 ** 255, 2 ** 256 - 1)]))

    # launch shapes
    good = []
    for _ in range(33):
        sd, m = rb(32), rb(32)
        good.append((ed.public_key(sd), m, ed.sign(sd, m), 2))
    for n in (1, 15, 16, 17, 33):
        out.append(("n = %d, all valid" % n, good[:n]))
    nokey = []
    while len(nokey) < 16:
        k = rb(32)
        if not ed.key_decodes(k):
            nokey.append((k, rb(32), rb(64), 0))
    early = [(k, m, with_s(s, int.from_bytes(s[32:], "little") + ed.L), 1) for k, m, s, _ in good[:16]]
    for name, fill in (("keys that do not decode", nokey), ("S >= L", early)):
        for j in range(16):
            out.append(("one valid signature at quad %d among %s" % (j, name), fill[:j] + [good[j]] + fill[j + 1:]))
    out.append(("a wave of early-outs, then a wave of valid signatures", nokey[:8] + early[8:] + good[16:32]))
    bad16 = (good[15][0], good[15][1], good[16][2], 1)           # the 16th carries the 17th's signature
    out.append(("17 signatures, the 16th invalid, the last valid", good[:15] + [bad16, good[16]]))
    assert expect(*bad16[:3]) == 1
    return out
