"""Seeded inputs for the three SHA routines (csrc/sha256.hip.h sha256_batch_kernel and sha256_pair_group, csrc/verdict.hip.h
sha_lane), shared by the CPU model (test_sha_order_model.py) and the GPU tests (test_gpu_sha_edges.py).

Block level: messages for zke_sha256_batch, laid back to back so that every length of EDGE_LENS starts at every offset
modulo 16 (the 16-byte load path and the byte-load path of a last chunk of 1..15 bytes at every alignment).
Pipeline level: e-mails signed by the independent Python signer (synth.sign_email) whose hashed body length and header
preimage length are set exactly; both algorithms, both body canonicalisations.  The expected digests are the signer's
(hashlib); nothing here looks at the engine."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

import synth
from synth import SignSpec, sign_email
from zkemail_rs_amd._abi import Email, PublicKey

SHA_TILE = 128                       # csrc/engine.hip: bytes of a message per LDS tile (two SHA blocks)
TILE_MULTIPLES = [128 * k for k in range(1, 9)] + [4096, 65536, 1048576]


def _edge_lens() -> List[int]:
    s = set(range(0, 301))
    for m in TILE_MULTIPLES:          # m - 10 .. m + 1: len % 64 of 54..63, 0, 1; at m - 8 .. m - 1 the 0x80 lies in one
        s.update(range(m - 10, m + 2))  # tile and the bit length in the next
    s.update((1500, 70000, 100003, 131072 + 57))      # a few long ones
    return sorted(s)


EDGE_LENS = _edge_lens()
PIPE_BODY_LENS = [n for n in EDGE_LENS if n <= 4097]       # the verdict launch's one-lane routine: bodies up to 4 097 bytes


# ------------------------------------------------------------------ block level
N_BLOCK = 32768 + 256 + 100          # above the 512-group threshold; the last workgroup: one full wave, one of 36 messages, two empty
N_BLOCK_CUT = 16384 + 100            # the same edge messages below the threshold (for a forced one-wave launch)
def _bytes(rng, n: int) -> bytes:
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def aligned_messages(seed: int = 7, lens: Sequence[int] = EDGE_LENS, aligns: Sequence[int] = tuple(range(16))) -> Tuple[List[bytes], List[int]]:
    """-> (messages, starts): for every alignment a and every length, a filler message of 0..15 bytes and then the message
    itself, which starts at a byte offset = a (mod 16) of the concatenation."""
    rng = np.random.default_rng(seed)
    msgs: List[bytes] = []
    starts: List[int] = []
    pos = 0
    for a in aligns:
        for n in lens:
            fill = (a - pos) % 16
            msgs.append(_bytes(rng, fill)); starts.append(pos); pos += fill
            msgs.append(_bytes(rng, n)); starts.append(pos); pos += n
    return msgs, starts


def wave_populations(seed: int = 8) -> List[Tuple[str, List[int]]]:
    """Lengths of 64 consecutive messages that one wave hashes in lock-step."""
    rng = np.random.default_rng(seed)
    pops = []
    for lane in (0, 63, 29):
        lens = [int(x) for x in rng.integers(0, 120, 64)]
        lens[lane] = 70000 + lane
        pops.append((f"one_long_lane{lane}", lens))
    pops.append(("all_empty", [0] * 64))
    pops.append(("one_block_apart", [64 * k + 55 - (k & 1) * 9 for k in range(64)]))      # nblk = k + 1 for lane k
    pops.append(("tile_staggered", [120 + 128 * (k % 5) + (k % 9) for k in range(64)]))   # rows finish in different tiles
    return pops


def block_message_set(n_total: int, seed: int = 7, max_len: Optional[int] = None) -> Tuple[List[bytes], dict]:
    """n_total messages: the aligned edge messages, the wave populations (each from a message index that is a multiple of
    64), then short random messages.  info: 'n_edge' = messages that must be kept when the set is cut, 'pops' = (name, first
    message) of each wave population."""
    lens = [n for n in EDGE_LENS if max_len is None or n <= max_len]
    msgs, _ = aligned_messages(seed, lens)
    rng = np.random.default_rng(seed + 1000)
    pops = []
    for name, pl in wave_populations(seed + 1):
        while len(msgs) % 64:
            msgs.append(_bytes(rng, int(rng.integers(0, 16))))
        pops.append((name, len(msgs)))
        msgs += [_bytes(rng, n) for n in pl]
    n_edge = len(msgs)
    assert n_edge <= n_total, (n_edge, n_total)
    fill = rng.integers(0, 301, n_total - n_edge)
    msgs += [_bytes(rng, int(n)) for n in fill]
    return msgs, {"n_edge": n_edge, "pops": pops}


# ------------------------------------------------------------------ e-mails
def domain_of_len(n: int) -> str:
    """A domain name of exactly n bytes (labels of at most 63)."""
    assert n >= 9
    body = n - 4                                  # ".com"
    labels = []
    while body > 40:
        labels.append("m" * 30); body -= 31
    labels.append("d" * body)
    d = ".".join(labels) + ".com"
    assert len(d) == n
    return d


def _headers(tag: int, domain: str, subject_pad: int = 0):
    """Fixed headers (the same bytes for every tag of the same decimal width) whose Subject — a signed header — is padded."""
    return [
        (b"Received", b"from mail.example.net by mx.example.net; Tue, 03 Oct 2026 10:00:00 +0000"),
        (b"From", f"Edge Case <edge@{domain}>".encode()),
        (b"To", b"Recipient <rcpt@example.net>"),
        (b"Subject", b"sha-edge-" + b"s" * subject_pad),
        (b"Date", b"Tue, 03 Oct 2026 10:00:00 +0000"),
        (b"Message-ID", f"<{tag:08d}@{domain}>".encode()),
    ]


def edge_email(rng, tag: int, body_len: int, algo: str = "rsa-sha256", body_canon: str = "relaxed", subject_pad: int = 0,
               domain: str = "example.com", key=None, l_short: bool = False, corrupt: Optional[str] = None, selector: str = "sel1"):
    """-> (Email, inter): an e-mail whose hashed body is exactly body_len bytes.  relaxed with body_len >= 3: a body whose
    canonical form has that length; otherwise (and always with l_short) a longer body cut by l=."""
    key = key or synth.load_keys()["rsa2048_00"]
    use_l = l_short or body_len < 3 or body_canon == "simple"
    body = synth.ascii_body(rng, body_len + 41 if use_l else body_len)
    spec = SignSpec(domain=domain, selector=selector, algo=algo, body_canon=body_canon, length=body_len if use_l else None)
    raw, it = sign_email(_headers(tag, domain, subject_pad), body, key, spec, corrupt=corrupt)
    assert it["hashed_body_len"] == body_len
    it["corrupt"] = corrupt
    it["algo"] = algo
    return Email(domain, raw, PublicKey(key.pkcs1_der)), it


ALGOS = ("rsa-sha256", "rsa-sha1")
CANONS = ("relaxed", "simple")


def interleave_check(inter) -> None:
    """every group of 64 consecutive e-mails holds both algorithms"""
    for g in range(0, len(inter), 64):
        assert len({it["algo"] for it in inter[g:g + 64]}) == 2 or len(inter) - g < 2, g


def body_sweep(lens: Sequence[int] = PIPE_BODY_LENS, seed: int = 31, extra_long: bool = True):
    """Every body length under both algorithms (neighbours in the batch: a=rsa-sha256, a=rsa-sha1), the canonicalisation
    alternating from pair to pair; with extra_long also the lengths around 65 536 and 1 048 576 (one e-mail each, the algorithm
    alternating).  -> (emails, inter)"""
    rng = np.random.default_rng(seed)
    emails, inter = [], []
    for k, n in enumerate(lens):
        for a in ALGOS:
            e, it = edge_email(rng, len(emails), n, a, CANONS[k & 1])
            emails.append(e); inter.append(it)
    if extra_long:
        for k, n in enumerate(x for x in EDGE_LENS if x > 4097):
            e, it = edge_email(rng, len(emails), n, ALGOS[k & 1], CANONS[(k >> 1) & 1])
            emails.append(e); inter.append(it)
    return emails, inter


HDR_SWEEP = 256


_OVERHEAD = {}


def _preimage_overhead(body_len: int, algo: str, body_canon: str) -> int:
    """header preimage bytes of an edge_email with an unpadded Subject (depends on the tags: a=, l=, the width of bh=)"""
    k = (body_len, algo, body_canon)
    if k not in _OVERHEAD:
        _OVERHEAD[k] = len(edge_email(np.random.default_rng(0), 0, body_len, algo, body_canon)[1]["canon_header"])
    return _OVERHEAD[k]


def header_sweep(seed: int = 32, body_lens: Sequence[int] = (55, 56, 63, 64, 119), count: int = HDR_SWEEP, first: int = 952):
    """Header preimages of exactly first .. first + count - 1 bytes (the signed Subject grows) under both algorithms.  With
    the defaults the preimages are 952 .. 1 207 bytes — length classes 16 and 17 — and the bodies fall into classes 1 and 2:
    a batch that keeps the direct lane -> job mapping in both kinds.  -> (emails, inter)"""
    rng = np.random.default_rng(seed)
    emails, inter = [], []
    for k in range(count):
        for a in ALGOS:
            bl, bc = body_lens[k % len(body_lens)], CANONS[(k >> 1) & 1]
            e, it = edge_email(rng, len(emails), bl, a, bc, subject_pad=first + k - _preimage_overhead(bl, a, bc))
            assert len(it["canon_header"]) == first + k
            emails.append(e); inter.append(it)
    return emails, inter


def domain_edge_emails(seed: int = 33):
    """from_domain (= d=) of 55, 56, 63 and 64 bytes: the padding edges of the from_domain hash (a kind 2 message)."""
    rng = np.random.default_rng(seed)
    emails, inter = [], []
    for n in (55, 56, 63, 64):
        for a in ALGOS:
            e, it = edge_email(rng, len(emails), 100 + n, a, domain=domain_of_len(n))
            emails.append(e); inter.append(it)
    return emails, inter


def pipeline_population():
    """The batch of GPU test 3: body sweep, header sweep and the domain edges in one batch."""
    parts = [body_sweep(), header_sweep(), domain_edge_emails()]
    emails = [e for p in parts for e in p[0]]
    inter = [i for p in parts for i in p[1]]
    return emails, inter


# ------------------------------------------------------------------ length-bucket populations
def _base_emails(specs, seed: int):
    """one signed e-mail per (body_len, subject_pad, algo, corrupt)"""
    rng = np.random.default_rng(seed)
    return [edge_email(rng, k, n, a, subject_pad=p, corrupt=c) for k, (n, p, a, c) in enumerate(specs)]


def repeat_emails(base, order: Sequence[int]):
    """A batch that repeats the signed e-mails `base` in the given order, each copy with a header of its own in front of the
    signature (X-Copy is not signed, so every copy still verifies).  -> (emails, inter)"""
    emails, inter = [], []
    for j, b in enumerate(order):
        e, it = base[b]
        emails.append(Email(e.from_domain, b"X-Copy: %d\r\n" % j + e.raw_email, e.public_key))
        inter.append(it)
    return emails, inter


def bucket_populations():
    """name -> (emails, inter) for GPU test 4; test_sha_order_model.py certifies what each one reaches."""
    out = {}
    # body classes 1 and 2 only, the two counters in different lanes' triples (lane 0 holds classes 0..2, lane 1 classes 3..5:
    # so classes 2 and 3) -> direct mapping with hi - lo == 1
    base = _base_emails([(119, 0, "rsa-sha256", None), (120, 0, "rsa-sha1", None), (150, 0, "rsa-sha256", None)], 41)
    out["direct_two_classes"] = repeat_emails(base, [k % 3 for k in range(300)])
    # classes 2 and 4 only: hi - lo == 2, the smallest spread that takes the bucketed mapping
    base = _base_emails([(100, 0, "rsa-sha256", None), (200, 0, "rsa-sha1", None), (230, 0, "rsa-sha256", None)], 42)
    out["bucketed_spread_two"] = repeat_emails(base, [(k * 7) % 3 for k in range(333)])
    # many classes, among them classes >= 16, groups that straddle three classes and more, n = 700 (not a multiple of 256,
    # cut groups), with invalid e-mails (no message of either kind: SHA_KEY_NONE) spread over the batch
    specs = []
    lens = [0, 55, 56, 119, 120, 300, 500, 959, 1000, 1500, 2100, 3000, 4097, 9000, 20000, 70000]
    for k, n in enumerate(lens):
        specs.append((n, 10 * k, ALGOS[k & 1], None))
    base = _base_emails(specs, 43)
    rng = np.random.default_rng(44)
    order = [int(x) for x in rng.integers(0, len(base), 700)]
    emails, inter = repeat_emails(base, order)
    for j in range(0, 700, 9):               # e-mails the front end finishes without a hash job: no blank line, no signature
        emails[j] = Email("example.com", b"From: a@example.com\r\nSubject: x %d" % j, emails[j].public_key)
        inter[j] = None
    out["ragged_with_invalid"] = (emails, inter)
    # fewer messages than groups: a batch of 130 e-mails of which 100 have no message — the bucketed groups beyond the total skip
    base = _base_emails([(60, 0, "rsa-sha1", None), (700, 0, "rsa-sha256", None), (5000, 0, "rsa-sha1", None)], 45)
    emails, inter = repeat_emails(base, [k % 3 for k in range(130)])
    for j in range(130):
        if j % 13 >= 3:
            emails[j] = Email("example.com", b"From: a@example.com\r\nSubject: y %d" % j, emails[j].public_key)
            inter[j] = None
    out["skipped_groups"] = (emails, inter)
    return out


def uniform_batch(n: int = 200, seed: int = 46):
    base = _base_emails([(333, 0, "rsa-sha256", None)], seed)
    return repeat_emails(base, [0] * n)


# ------------------------------------------------------------------ the model's view of a population
def nblk(length: int) -> int:
    return (length + 9 + 63) >> 6


def population_lengths(inter):
    """[(body_len, header_len, sha1) or None]: what the front end files for each e-mail"""
    return [None if it is None else (it["hashed_body_len"], len(it["canon_header"]), it["algo"] == "rsa-sha1") for it in inter]


# ------------------------------------------------------------------ later signature rounds (verdict.hip.h, sha_lane)
def signature_round_emails(body_lens: Sequence[int] = PIPE_BODY_LENS, hdr_count: int = 130, seed: int = 51):
    """E-mails with one or three failing same-domain signatures in front of the good one, so that the good signature's body
    and header preimage are hashed by the verdict launch's one-lane routine.  Every body length under both algorithms (l=
    shorter than the body, c=relaxed and c=simple alternating), then hdr_count consecutive header-preimage lengths under both
    algorithms.  -> (cases, n_bad per case)"""
    import cases
    rng = np.random.default_rng(seed)
    out, nbad = [], []
    for k, n in enumerate(body_lens):
        for j, a in enumerate(ALGOS):
            nb = 1 if (k + j) & 1 else 3
            c = cases.multi_signature_case(nb, body=synth.ascii_body(rng, n + 41), spec=SignSpec(algo=a, body_canon=CANONS[(k >> 1) & 1], length=n))
            c.inter["algo"] = a
            out.append(c); nbad.append(nb)
    for k in range(hdr_count):
        for j, a in enumerate(ALGOS):
            nb = 3 if (k + j) & 1 else 1
            c = cases.multi_signature_case(nb, body=synth.ascii_body(rng, 63 + 41), spec=SignSpec(algo=a, body_canon=CANONS[k & 1], length=63),
                                           hdr_pad=k + 1 + (k & 1))          # ("c=relaxed/simple" is a byte shorter than "c=relaxed/relaxed")
            c.inter["algo"] = a
            out.append(c); nbad.append(nb)
    return out, nbad
