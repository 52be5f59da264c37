"""remove_quoted_printable_soft_breaks (core/src/email.rs:61-86) with BOTH return values, restated in Python; the wave formulation of
csrc/qpmap.hip.h (64-byte steps, the 3-byte pattern as shifted ballots, 1 or 2 dropped bytes carried into the next step); the origin
rule of zke_extract_captures_mapped (include/zkemail_amd.h); and the case list the CPU and GPU tests share."""
import random

NO_INDEX = 0xFFFFFFFF
ORGF_SPLIT, ORGF_PADDING = 1, 2
SOFT = b"=\r\n"


def remove_qp(body: bytes):
    """email.rs:61-86: (cleaned zero-padded to len(body), index_map padded with NO_INDEX, bytes kept)."""
    n, i = len(body), 0
    cleaned, im = bytearray(), []
    while i < n:
        if body[i:i + 3] == SOFT:                       # email.rs:69-71
            i += 3
        else:
            cleaned.append(body[i])
            im.append(i)
            i += 1
    kept = len(cleaned)
    return bytes(cleaned) + bytes(n - kept), im + [NO_INDEX] * (n - kept), kept


def keep_masks(body: bytes, step: int = 64):
    """Per step of `step` bytes: (base, keep mask) as qp_keep_mask computes them — D = lanes where "=\\r\\n" begins, drop = D | D << 1 |
    D << 2 plus the carry of the previous step, carry = 2 if the last lane begins a break, 1 if the last but one does."""
    n, carry, full = len(body), 0, (1 << step) - 1
    for base in range(0, n, step):
        D = 0
        for lane in range(step):
            if body[base + lane:base + lane + 3] == SOFT:
                D |= 1 << lane
        drop = (D | (D << 1) | (D << 2)) & full
        drop |= 3 if carry == 2 else (1 if carry == 1 else 0)
        carry = 2 if (D >> (step - 1)) & 1 else (1 if (D >> (step - 2)) & 1 else 0)
        keep = 0
        for lane in range(step):
            if base + lane < n and not (drop >> lane) & 1:
                keep |= 1 << lane
        yield base, keep


def ballot_remove_qp(body: bytes, step: int = 64):
    """qp_index_kernel: every kept lane stores its byte and its position at o + popcount(keep below the lane)."""
    n = len(body)
    cleaned, im, o = bytearray(n), [NO_INDEX] * n, 0
    for base, keep in keep_masks(body, step):
        for lane in range(step):
            if (keep >> lane) & 1:
                at = o + bin(keep & ((1 << lane) - 1)).count("1")
                cleaned[at], im[at] = body[base + lane], base + lane
        o += bin(keep).count("1")
    return bytes(cleaned), im, o


def select(mask: int, r: int) -> int:
    """Position of the r-th set bit."""
    pos = 0
    while True:
        if (mask >> pos) & 1:
            if r == 0:
                return pos
            r -= 1
        pos += 1


def ballot_lookup(body: bytes, queries, step: int = 64):
    """capture_origin_kernel's walk: im[q] for every q of `queries` without a map — a query q with o <= q < o + popcount(keep) resolves
    to base + select(keep, q - o); what is at or beyond the final o stays NO_INDEX."""
    res, o = [NO_INDEX] * len(queries), 0
    for base, keep in keep_masks(body, step):
        cnt = bin(keep).count("1")
        for k, q in enumerate(queries):
            if o <= q < o + cnt:
                res[k] = base + select(keep, q - o)
        o += cnt
    return res


def origin(im, n: int, s: int, e: int):
    """The origin of span {s, e} of the cleaned haystack (n bytes, index map im): (start, end, flags)."""
    if s == NO_INDEX and e == NO_INDEX:                 # an e-mail without strings
        return s, e, 0
    start = im[s] if s < n else NO_INDEX
    if e == s:
        end = start
    else:
        end = NO_INDEX if im[e - 1] == NO_INDEX else im[e - 1] + 1
    if start == NO_INDEX or end == NO_INDEX:
        return start, end, ORGF_PADDING
    return start, end, (ORGF_SPLIT if end - start != e - s else 0)


LENGTHS = [0, 1, 2, 3] + list(range(61, 68)) + list(range(127, 131)) + [4096]
ALPHABET = [b"=", b"\r", b"\n", b"a", SOFT]


def seeded_bodies(count: int, seed: int):
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        n = rng.choice(LENGTHS)
        out.append(b"".join(rng.choice(ALPHABET) for _ in range(n))[:n])
    return out


def cases(seeded: int = 2000):
    """Bodies at which a 64-byte-step compaction can go wrong (the list of the issue that introduced the index map)."""
    out = [bytes((7 * k + 33) % 95 + 32 for k in range(n)).replace(b"=", b"a") for n in LENGTHS]     # every length, no break
    big = bytearray(b"abcdefghij" * 6554)[:65537]                          # 65 537 bytes: 1 025 steps, breaks at both ends of steps
    for at in (0, 61, 126, 191, 4093, 32767, 65470, 65534):
        big[at:at + 3] = SOFT
    out.append(bytes(big))
    for step_at in (61, 62, 63, 64):                                       # a break that starts at byte 61 .. 64 of a step: carry 0, 1, 2, 0
        for steps in (1, 2):
            at = 64 * (steps - 1) + step_at
            out.append(b"a" * at + SOFT + b"b" * 70)
            out.append(b"a" * at + SOFT)                                   # ... and as the last three bytes
    out += [b"abc" + SOFT, SOFT, b"abc=\r", b"abc=", b"=\r", b"=", b"a" * 62 + b"=\r", b"a" * 63 + b"="]      # "=\r" and "=" at the end: no break
    out += [SOFT * k for k in (2, 21, 22, 43, 100)]                        # nothing but soft breaks: clean_len 0
    out += [b"x" * k + SOFT * r + b"y" * 5 for k in (0, 59, 60, 61, 62, 63) for r in (2, 3, 22)]              # runs across step boundaries
    out += [b"=\r=\r\n\n", b"==\r\n\r\n", b"=\r\n\r\n=", b"\r\n=\r\n=\r\n="]
    return out + seeded_bodies(seeded, 20261019)
