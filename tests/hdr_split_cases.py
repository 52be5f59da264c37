"""Seeded populations that walk the header split of csrc/hdrsplit.hip.h (split_headers_lines, scan_headers, find_body) through
its geometry: every lane of a 64-byte chunk, the chunk and line-group edges, the 64-entry span table, the LINE_CAP and
ZKE_MAX_HEADERS limits and the staged edge at byte 3 568.  No engine and no oracle in here: tests/test_hdr_split_model.py
certifies on the CPU what each population reaches, tests/test_gpu_hdr_split.py runs them on the device.
(cases.fold_offset_emails sweeps the canonicaliser's scan of header VALUES; this file sweeps the split in front of it.)

Every population is a list of (name, raw, from_domain).
"""
from __future__ import annotations

import itertools
from typing import Dict, List, Tuple

import numpy as np

from zkemail_rs_amd._abi import Email, PublicKey

import synth
from synth import SignSpec, sign_email

DOMAIN = "example.com"
STAGE = 3568
Case = Tuple[str, bytes, str]

# every kind of line once; three headers NAMED DKIM-Signature (one folded) whose spans the scan entry reports
TAIL = (b"K: v\r\n"
        b"Fold-Sp: first\r\n second\r\n"
        b"DKIM-Signature: not a tag list\r\n"
        b"Fold-Tab: first\r\n\tsecond\r\n"
        b"a line without colon\r\n"
        b"\tTab-Key: directly behind it\r\n"
        b"Bare-Lf: ended by LF alone\n"
        b"Cr-Cr: ended by CR CR LF\r\r\n"
        b"Empty-Value:\r\n"
        b"dkim-signature: v=1; folded\r\n\th=a:b; colon in the continuation\r\n  \r\n"
        b"Spaces-Only:    \r\n"
        b"Colon-In-Fold: a\r\n b: c\r\n"
        b"K::: a:b\r\n"
        b"DKIM-SIGNATURE:   d=example.com  \r\n")
# the same kinds under X- names, for the front of a signed message (no second DKIM-Signature there)
X_TAIL = (b"X-K: v\r\n"
          b"X-Fold-Sp: first\r\n second\r\n"
          b"X-Fold-Tab: first\r\n\tsecond\r\n"
          b"X-a line without colon\r\n"
          b"\tX-Tab-Key: directly behind it\r\n"
          b"X-Bare-Lf: ended by LF alone\n"
          b"X-Cr-Cr: ended by CR CR LF\r\r\n"
          b"X-Empty-Value:\r\n"
          b"X-Spaces-Only:    \r\n"
          b"X-Colon-In-Fold: a\r\n b: c\r\n"
          b"X-K::: a:b\r\n")
SPELLINGS = {"crlf_crlf": (b"\r\n", b"\r\n"), "lf_lf": (b"\n", b"\n"), "lf_crlf": (b"\n", b"\r\n"), "crlf_lf": (b"\r\n", b"\n")}
BODY = b"first body line\r\nsecond\r\n\r\nbehind an empty body line\r\n"


def offset_sweep() -> List[Case]:
    """X-P: p*s, the tail, a last header, the empty line in its four spellings, a body; s = 0..127: every LF, every first ':'
    and the cut pass through every lane, lanes 62 / 63 put the look-ahead into the next chunk."""
    out = []
    for s in range(128):
        for sp, (end, empty) in SPELLINGS.items():
            raw = b"X-P: " + b"p" * s + b"\r\n" + TAIL + b"Last: z" + end + empty + BODY
            out.append((f"sweep_{s}_{sp}", raw, DOMAIN))
    return out


# ------------------------------------------------------------------ line counts
LINE_COUNTS = (63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513)
HDR, CONT, KEYONLY, SPLINE, TABHDR, LONECR = b"k:v\r\n", b" c\r\n", b"kk\r\n", b" x\r\n", b"\tc:d\n", b"\rx\r\n"
SIGHDR = b"DKIM-Signature:v\r\n"              # a header line whose span the scan entry reports (a few per block)


def _block(lines_: List[bytes]) -> bytes:
    assert all(len(ln) <= 6 or ln.startswith(SIGHDR[:15]) for ln in lines_)
    block = b"".join(lines_)
    assert len(block) + 2 <= STAGE and 0 < sum(ln.startswith(SIGHDR[:15]) for ln in lines_) <= 64
    return block + b"\r\n" + BODY


def _pattern(n: int, per: int) -> List[bytes]:
    """n lines: headers of `per` lines each (one header line, per - 1 continuation lines); the header lines at the multiples
    of 63 and 64 are named DKIM-Signature."""
    return [CONT if i % per else SIGHDR if i % 63 == 0 or i % 64 == 0 else HDR for i in range(n)]


def line_counts() -> List[Case]:
    """Blocks of LINE_COUNTS lines of at most 6 bytes, a few named header lines apart (they fit the staged part), as one-line headers (255 / 256 / 257
    headers among them) and as three-line headers; line 64 (and 128), the first of a line group, as (a) a continuation of
    a header with a value, (b) a SP line behind a key-only line, (c) an HTAB line behind a key-only line, (d) a new header;
    headers 63 / 64 / 65 whose last continuation line opens the next line group; `leading space` and lone CR in front of
    and behind the 257th header start, and against each other."""
    out = []
    for n in LINE_COUNTS:
        for per in (1, 3):
            out.append((f"lines_{n}_per{per}", _block(_pattern(n, per)), DOMAIN))
            for edge in (64, 128):
                if n <= edge:
                    continue
                for tag, before, at in (("a_cont", SIGHDR, CONT), ("b_sp_after_keyonly", KEYONLY, SPLINE), ("c_tab_after_keyonly", KEYONLY, TABHDR),
                                        ("d_header", HDR, SIGHDR)):
                    ls = _pattern(n, per)
                    ls[edge - 1], ls[edge] = before, at
                    out.append((f"lines_{n}_per{per}_line{edge}_{tag}", _block(ls), DOMAIN))
    for h, edge in ((63, 64), (64, 128), (65, 128)):
        # headers 0 .. h - 1 fill lines 0 .. edge - 2 (header 0 takes the spare lines), header h starts on line edge - 1
        ls = [HDR] + [CONT] * (edge - 1 - h) + [HDR] * (h - 1) + [SIGHDR, CONT] + [HDR] * 5
        assert len(ls) == edge + 6
        out.append((f"header_{h}_ends_on_line_{edge}", _block(ls), DOMAIN))
        ls2 = list(ls)
        ls2[edge - 1] = b"DKIM-Signature: \r\n"                     # spaces only, then a continuation that holds only CR
        ls2[edge] = b"\t\r\r\n"
        out.append((f"header_{h}_ends_on_line_{edge}_blank_value", _block(ls2), DOMAIN))
    out.append(("err_lead_then_257th_header", _block([SIGHDR] + [HDR] * 254 + [KEYONLY, SPLINE, HDR, HDR]), DOMAIN))
    out.append(("err_257th_header_then_lead", _block([SIGHDR] + [HDR] * 255 + [KEYONLY, SPLINE, HDR]), DOMAIN))
    out.append(("err_lonecr_then_257th_header", _block([SIGHDR] + [HDR] * 254 + [LONECR, HDR, HDR]), DOMAIN))
    out.append(("err_257th_header_then_lonecr", _block([SIGHDR] + [HDR] * 255 + [HDR, LONECR, HDR]), DOMAIN))
    out.append(("err_lead_then_lonecr", _block([SIGHDR] + [HDR] * 69 + [KEYONLY, SPLINE, LONECR, HDR]), DOMAIN))
    out.append(("err_lonecr_then_lead", _block([SIGHDR] + [HDR] * 69 + [LONECR, KEYONLY, SPLINE, HDR]), DOMAIN))
    out.append(("err_lead_alone_line_0", _block([SPLINE] + [HDR] * 3 + [SIGHDR]), DOMAIN))
    out.append(("err_lonecr_alone_line_63", _block([SIGHDR] + [HDR] * 62 + [LONECR] + [HDR] * 3), DOMAIN))
    out.append(("err_lead_in_a_later_group_than_lonecr", _block([SIGHDR] + [HDR] * 59 + [LONECR] + [HDR] * 9 + [KEYONLY, SPLINE]), DOMAIN))
    out.append(("ok_256_headers_then_continuations", _block([HDR] * 255 + [SIGHDR] + [CONT] * 70), DOMAIN))
    return out


# ------------------------------------------------------------------ the staged edge
EDGE_POSITIONS = range(3560, 3573)
STAGED_EDGE_ROUTE: Dict[str, str] = {}      # name -> the route the geometry implies (filled by staged_edge())
_EDGE_HEAD = b"From: a@example.com\r\nDKIM-Signature: front\r\nSubject: staged\r\n edge\r\n"


def _pad_line(total: int) -> bytes:
    """An X-Pad header line of exactly `total` bytes."""
    assert total >= 9
    return b"X-Pad: " + b"p" * (total - 9) + b"\r\n"


def staged_edge() -> List[Case]:
    """The LF that closes the last header at 3 560..3 572 in the four spellings of the empty line, the e-mail ending right
    behind it or going on with a body; the ':' of a header named DKIM-Signature, its fold and its value end at the same
    positions with the empty line further on (the serial walk, straddling LDS and HBM); whole e-mails of 3 552, 3 567,
    3 568, 3 569 and 3 584 bytes (the staging copy's 16-byte tail)."""
    out = []
    STAGED_EDGE_ROUTE.clear()

    def add(name, raw, route):
        out.append((name, raw, DOMAIN))
        STAGED_EDGE_ROUTE[name] = route

    for P in EDGE_POSITIONS:
        for sp, (end, empty) in SPELLINGS.items():
            last = b"Last: z" + end
            head = _EDGE_HEAD + _pad_line(P + 1 - len(_EDGE_HEAD) - len(last)) + last
            assert len(head) == P + 1 and head[P] == 10
            for tail_name, tail in (("ends", b""), ("body", BODY)):
                raw = head + empty + tail
                look = P + len(empty)                   # the last byte the cut's look-ahead reads
                add(f"edge_lf_{P}_{sp}_{tail_name}", raw, "lines" if look < min(len(raw), STAGE) else "serial")
        sig = b"DKIM-Signature: v=1; at the edge\r\n\tfolded: part\r\n"
        rest = b"After-The-Edge: the empty line lies beyond the staged part\r\n\r\n" + BODY
        for what, at in (("colon", 14), ("fold", sig.index(b"\n")), ("value_end", len(sig) - 2)):
            front = _EDGE_HEAD + _pad_line(P - at - len(_EDGE_HEAD))
            raw = front + sig + rest
            assert len(front) + at == P
            add(f"edge_{what}_{P}", raw, "serial")
    for L in (3552, 3567, 3568, 3569, 3584):
        last = b"Last: z\r\n\r\n"
        raw = _EDGE_HEAD + _pad_line(L - len(_EDGE_HEAD) - len(last)) + last
        assert len(raw) == L
        add(f"whole_{L}_ends_with_the_empty_line", raw, "lines" if L - 1 < min(L, STAGE) else "serial")
        raw = _EDGE_HEAD + b"\r\n" + (BODY * 80)[:L - len(_EDGE_HEAD) - 2]
        assert len(raw) == L
        add(f"whole_{L}_body_to_the_end", raw, "lines")
        raw = _EDGE_HEAD + _pad_line(L - len(_EDGE_HEAD) - 7) + b"Last: z"
        assert len(raw) == L
        add(f"whole_{L}_no_empty_line", raw, "serial")
    return out


# ------------------------------------------------------------------ short and unterminated
def short_inputs() -> List[Case]:
    """Every input of 0..3 bytes over {LF, CR, SP, HTAB, ':', 'a'}; inputs without an empty line that end inside a key,
    inside a value, on LF, on LF SP, on CR."""
    out = []
    for n in range(4):
        for t in itertools.product(b"\n\r \t:a", repeat=n):
            raw = bytes(t)
            out.append(("short_" + (raw.hex() or "empty"), raw, DOMAIN))
    for name, end in (("in_key", b"Unfinished-Ke"), ("in_value", b"Key: unfinished val"), ("on_lf", b"Key: v\n"), ("on_crlf", b"Key: v\r\n"),
                      ("on_lf_sp", b"Key: v\n "), ("on_lf_tab", b"Key: v\r\n\t"), ("on_cr", b"Key: v\r"), ("on_lf_cr", b"Key: v\n\r"),
                      ("on_colon", b"Key:"), ("on_colon_spaces", b"Key:   "), ("keyonly_then_cr", b"Key\n\r")):
        out.append((f"unterminated_{name}", TAIL + end, DOMAIN))
        out.append((f"unterminated_{name}_alone", end, DOMAIN))
    return out


# ------------------------------------------------------------------ find_body
def _filler(k: int) -> bytes:
    """k bytes with CR, LF, CRLF and CRLFCR decoys in them but no CRLFCRLF, not ending in CR or LF."""
    pat = b"ab\r\n\rcd\re\nf\r\n\r\rg\n\r\nh"
    f = (pat * (k // len(pat) + 1))[:k]
    return f[:-2] + b"xy"[:min(2, k)] if k >= 2 else b"x" * k


def find_body_cases() -> List[Case]:
    """A header list ended by LF.LF or LF.CRLF with the first CRLFCRLF d = 0..130 bytes behind hdr_end (the device walks
    64-byte windows in steps of 61), and the ends: no CRLFCRLF, CRLFCRLF as the last four bytes, CRLFCR as the last three,
    CRLFCRLF starting at 3 564..3 569."""
    out = []
    hdrs = b"From: a@example.com\r\nDKIM-Signature: x\r\nSubject: find the body\n"
    for sp, empty in (("lf_lf", b"\n"), ("lf_crlf", b"\r\n")):
        for d in range(131):
            if d == 0 and empty == b"\r\n":
                raw = hdrs + b"\r\n\r\n" + BODY
            elif d < len(empty) or (empty == b"\r\n" and d == 2):
                continue                                  # no first CRLFCRLF can start there: the empty line's own bytes decide
            else:
                raw = hdrs + empty + _filler(d - len(empty)) + b"\r\n\r\nthe body\r\n"
            assert raw.find(b"\r\n\r\n") == len(hdrs) + d, (sp, d)
            out.append((f"body_{sp}_d{d}", raw, DOMAIN))
        out.append((f"body_{sp}_none", hdrs + empty + _filler(200), DOMAIN))
        out.append((f"body_{sp}_last_four", hdrs + empty + _filler(100) + b"\r\n\r\n", DOMAIN))
        out.append((f"body_{sp}_crlfcr_last_three", hdrs + empty + _filler(100) + b"\r\n\r", DOMAIN))
        for at in range(3564, 3570):
            raw = hdrs + empty + _filler(at - len(hdrs) - len(empty)) + b"\r\n\r\nthe body\r\n"
            assert raw.find(b"\r\n\r\n") == at
            out.append((f"body_{sp}_at_{at}", raw, DOMAIN))
    return out


UNSIGNED = {"offset_sweep": offset_sweep, "line_counts": line_counts, "staged_edge": staged_edge, "short_inputs": short_inputs,
            "find_body": find_body_cases}
_UNSIGNED_CACHE: Dict[str, List[Case]] = {}


def unsigned(name: str) -> List[Case]:
    if name not in _UNSIGNED_CACHE:
        _UNSIGNED_CACHE[name] = UNSIGNED[name]()
    return _UNSIGNED_CACHE[name]


# ------------------------------------------------------------------ signed, three routes
SHIFTS = [(k * 11) % 128 for k in range(48)]
_SIGNED_CACHE = None


def _core_headers():
    return [(b"Received", b"from a.example.net\r\n\tby b.example.net; Tue, 03 Oct 2026 10:00:00 +0000"),
            (b"From", b"Alice <alice@example.com>"),
            (b"To", b"bob@example.net"),
            (b"Subject", b"split geometry,\r\n\tfolded once\r\n and twice"),
            (b"Date", b"Tue, 03 Oct 2026 10:00:00 +0000"),
            (b"Message-ID", b"<split@example.com>")]


def signed():
    """-> (cases, emails, intermediates, sig_index, route): one signed core per header canonicalisation (signed Subject
    folded), found by the split behind unsigned X- lines of the offset sweep's kinds — unsigned headers in front of a
    signature leave it valid — on three routes, 48 shifts each:
      L      the line path;
      S-hbm  one unsigned 3 584-byte X-Pad line first: the empty line lies beyond the staged part, the serial walk reads LDS
             and HBM;
      S-lds  one failing same-domain signature in front of the good one (its bh= is that of another body): the good one is
             split by the later round's serial walk, from LDS;
      S-hbm-later  (11 shifts) both of the above: an X-Pad line of 3 500 bytes and more, the failing signature across the staged
             edge, the good one beyond it — found by the later round, its value read from HBM;
    and 16 messages behind 56..63 one-line headers, whose signed headers land on entries 58..69 of the span table (both
    sides of entry 64).  Six signatures are made in all.  (The signer produces every shape asked for; none is left out.)"""
    global _SIGNED_CACHE
    if _SIGNED_CACHE is not None:
        return _SIGNED_CACHE
    key = synth.load_keys()["rsa2048_00"]
    pk = PublicKey(key.pkcs1_der)
    body = synth.ascii_body(np.random.default_rng(77), 333)
    other = synth.ascii_body(np.random.default_rng(78), 120)
    cs, emails, inter, sig_index, routes = [], [], [], [], []

    def add(name, raw, it, ix, route):
        cs.append((name, raw, DOMAIN))
        emails.append(Email(DOMAIN, raw, pk))
        inter.append(it)
        sig_index.append(ix)
        routes.append(route)

    for hc in ("relaxed", "simple"):
        hs = _core_headers()
        good, it = sign_email(hs, body, key, SignSpec(header_canon=hc))
        bad, _ = sign_email(hs, other, key, SignSpec(header_canon=hc, selector="old"))
        bad_sig = bad[:bad.find(b"Received:")]
        for s in SHIFTS:
            front = b"X-P: " + b"p" * s + b"\r\n" + X_TAIL
            add(f"signed_{hc}_L_{s}", front + good, it, 0, "L")
            add(f"signed_{hc}_S-hbm_{s}", _pad_line(3584) + front + good, it, 0, "S-hbm")
            add(f"signed_{hc}_S-lds_{s}", front + bad_sig + good, it, 1, "S-lds")
            if s < 24:
                add(f"signed_{hc}_S-hbm-later_{s}", _pad_line(3500 + s) + bad_sig + front + good, it, 1, "S-hbm-later")
        for k in range(56, 64):
            front = b"".join(b"X-F%d: %d\r\n" % (j, j) for j in range(k))
            add(f"signed_{hc}_behind_{k}_headers", front + good, it, 0, "L")
    _SIGNED_CACHE = (cs, emails, inter, sig_index, routes)
    return _SIGNED_CACHE


# ------------------------------------------------------------------ structured random blocks (CPU tier)
_KINDS = (b"K: v", b"Key-%d: value %d", b" folded with SP", b"\tfolded with HTAB", b"no colon here", b"\tTab: key", b"E:", b"S:   ",
          b" a: b in a fold", b"K::: a:b", b"DKIM-Signature: x", b"k:v", b" c", b"kk", b"\tc:d")
_ENDS = (b"\r\n", b"\r\n", b"\r\n", b"\n", b"\r\r\n")
_RARE = (b" lead", b"\rlone", b"\r", b" ")
_COUNTS = (0, 1, 2, 3, 62, 63, 64, 65, 66, 127, 128, 129, 130, 255, 256, 257, 258, 300, 511, 512, 513, 514)


def structured_blocks(n: int = 5000, seed: int = 20261019) -> List[Case]:
    """Seeded header blocks built line by line from the kinds above (an error line now and then, seldom enough for long
    valid blocks), line counts drawn from the edge list with a little jitter, the empty line in any spelling or missing."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        count = int(_COUNTS[int(rng.integers(0, len(_COUNTS)))])
        if rng.random() < 0.3:
            count = max(0, count + int(rng.integers(-2, 3)))
        small = count > 200 or rng.random() < 0.3          # short lines keep long blocks inside the staged part
        p_err = 0.0 if rng.random() < 0.6 else 0.5 / (count + 1)
        parts = []
        kind_ix = rng.integers(0, len(_KINDS), count)
        end_ix = rng.integers(0, len(_ENDS), count)
        errs = rng.random(count) < p_err
        in_value = False
        for j in range(count):
            k = int(kind_ix[j])
            if small:
                k = 11 + k % 4
            ln = _KINDS[k]
            if b"%d" in ln:
                ln = ln % (j, j)
            if ln[:1] == b" " and not in_value:            # a SP line is drawn only where it continues a value ...
                ln = _KINDS[11 if small else 0]
            if errs[j]:                                    # ... errors come from here, seldom
                ln = _RARE[int(rng.integers(0, len(_RARE)))] + ln
            in_value = in_value if ln[:1] in (b" ", b"\t") and in_value else b":" in ln
            parts.append(ln + _ENDS[int(end_ix[j])])
        r = rng.random()
        empty = b"" if r < 0.1 else (b"\r\n", b"\n")[int(rng.integers(0, 2))]
        pad = b"X-Pad: " + b"p" * int(rng.integers(0, 64)) + b"\r\n" if rng.random() < 0.5 else b""
        out.append((f"block_{i}", pad + b"".join(parts) + empty + (BODY if rng.random() < 0.7 else b""), DOMAIN))
    return out
