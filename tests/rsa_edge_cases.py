"""RSA operands that reach the data-dependent paths of the two device modexp routines, shared by the CPU models
(tests/test_rsa_wave_model.py, tests/test_rsa_group_model.py) and the GPU tests (tests/test_gpu_rsa_edges.py).
Deterministic and seeded; every case is (n, e, s, tag) and the tag names the path the case is there for.

The paths (csrc/rsa.hip.h, rsa_kernel.hip.h, rsa_quad.hip.h):
  * c0 — the 65th bit out of the first v_mad_u64_u32 of a CIOS step of the wave routine.  Random operands never set it;
    mont(X, X) with X < n = 2^k - c whose high limbs are all ones does.  X is reached from the signature X R^-1 mod n
    (R = 2^(2048 NL)): the routine's first product turns s into s R = X and its first squaring is mont(X, X).
  * the final EM + n -> EM subtraction of the lane-group routine: taken when s^65537 mod n is small against n, so
    s = t^d mod n for a small t (a key whose d is known).
  * the lane-group s >= n check, decided by the highest lane of the group that differs: n +- 2^(532 p) for lane p.
"""
import random

QL = 19
LANE_BITS = 28 * QL                                   # 532 bits per lane of a lane group
WAVE_EXPONENTS = (2, 3, 17, 65537, (1 << 32) + 1, (1 << 33) - 1)      # rsa 0.9.6 accepts 2 <= e < 2^33


def container_bits(bits):
    """the wave routine's R = 2^container: one 32-bit limb per lane up to 2048 bits, two up to 4096"""
    return 2048 if bits <= 2048 else 4096


def group_lanes(bits):
    """lanes per signature of the lane-group routine: four up to 2048 bits, eight up to 4096"""
    return 4 if bits <= 2048 else 8


def rand_odd(bits, rng):
    return rng.getrandbits(bits) | (1 << (bits - 1)) | 1


def moduli(seed=5):
    """-> [(tag, n)] of 512..4096 bits: the synthetic moduli of the issue's list, in a fixed order."""
    rng = random.Random(seed)
    out = []
    for k in (1024, 2048, 3072, 4096):
        out.append((f"ones{k}", (1 << k) - 1))                           # all-ones limbs
        out.append((f"smallest{k}", (1 << (k - 1)) + 1))                 # the smallest modulus of the length
    for k in (2048, 4096):
        c = rng.getrandbits(rng.randrange(600, 1501)) | 1
        out.append((f"2^{k}-c", (1 << k) - (c | (1 << (c.bit_length() - 1)))))
    for k in (2048, 4096):
        for lb in (LANE_BITS, 2 * LANE_BITS):                           # a 32-bit limb boundary on a lane boundary
            out.append((f"lane{lb}_{k}", (1 << (k - 1)) + (1 << lb) + 1))
    for bits in (1031, 1537, 2049, 2100):                               # the lane-group model's odd sizes
        out.append((f"odd{bits}", rand_odd(bits, rng)))
    for bits in (512, 513, 1023, 1025, 2047, 2048, 2049, 3071, 3073, 4095, 4096):    # container edges
        out.append((f"edge{bits}", rand_odd(bits, rng)))
    return out


def small_moduli(seed=6):
    """moduli below the lane-group routine's 512 bits, for the building-block entry only (zke_rsa_modexp_batch takes any odd
    modulus of 2 bits or more; so does the oracle)"""
    rng = random.Random(seed)
    return [("tiny3", 3), ("mersenne61", (1 << 61) - 1), ("tiny65", rand_odd(65, rng)), ("edge511", rand_odd(511, rng))]


def high_ones_x(n, rng):
    """X < n whose high 32-bit limbs are all ones (n = 2^k - c with c < 2^1501: X = n minus a value below c)"""
    c = (1 << n.bit_length()) - n
    return n - 1 - rng.randrange(max(c, 2))


def signatures(n, rng, G=None, with_rejects=True):
    """-> [(s, tag)]: the signature values of the case list for modulus n.  Rejected values (s >= n) are tagged 'reject-...'."""
    bits = n.bit_length()
    G = G or group_lanes(bits)
    R = 1 << container_bits(bits)
    out = [(0, "zero"), (1, "one"), (2, "two"), (n - 2, "n-2"), (n - 1, "n-1"), (rng.randrange(n), "random")]
    for p in range(G):
        if LANE_BITS * p < bits - 1:
            out.append((n - (1 << (LANE_BITS * p)), f"n-lane{p}"))     # accepted: lane p decides s < n
    if (1 << bits) - n < 1 << 1501:                                      # high limbs of n all ones: the c0 carry
        for _ in range(2):
            x = high_ones_x(n, rng)
            out.append((x * pow(R, -1, n) % n, "c0"))
    if with_rejects:
        out.append((n, "reject-n"))
        for p in range(G):
            out.append((n + (1 << (LANE_BITS * p)), f"reject-lane{p}"))  # rejected: lane p decides s > n
    return [(s, t) for s, t in out if s >= 0]


def small_result_signatures(key, rng):
    """s = t^d mod n for t some 200 to 300 bits shorter than n: s^e mod n = t is small, the lane-group routine's last
    product leaves t + n and the final subtraction runs (with borrows into the lanes where t + n carries; t = 2^m - 1
    carries out of every lane boundary below m)."""
    n, bits = key.n, key.n.bit_length()
    out = []
    for short in (200, 300):
        t = rng.getrandbits(bits - short) | (1 << (bits - short - 1))
        out.append((pow(t, key.d, n), f"small-t{bits - short}"))
    out.append((pow((1 << (bits - 250)) - 1, key.d, n), f"small-t-ones{bits - 250}"))
    return out


def wave_cases(seed=7, exponents=WAVE_EXPONENTS):
    """-> [(n, e, s, tag)] for the building-block entry (the wave routine): every modulus x every signature x one exponent
    of the list in turn, plus every exponent on n - 1, 2 and a c0 / random value."""
    rng = random.Random(seed)
    out = []
    for mi, (mt, n) in enumerate(moduli() + small_moduli()):
        sigs = signatures(n, rng) if n.bit_length() >= 512 else \
            [(0, "zero"), (1, "one"), (n - 1, "n-1"), (rng.randrange(n), "random"), (n, "reject-n")]
        for si, (s, st) in enumerate(sigs):
            e = exponents[(mi + si) % len(exponents)]
            out.append((n, e, s, f"{mt}/{st}/e{e}"))
        for e in exponents:
            for s, st in sigs:
                if st in ("n-1", "c0", "random"):
                    out.append((n, e, s, f"{mt}/{st}/e{e}"))
    return out


def key_cases(keys, names, seed=8):
    """-> [(n, e, s, tag)] under real keys (d known): small results and the shared signature list"""
    rng = random.Random(seed)
    out = []
    for name in names:
        k = keys[name]
        for s, st in small_result_signatures(k, rng) + signatures(k.n, rng):
            out.append((k.n, k.e, s, f"{name}/{st}"))
    return out
