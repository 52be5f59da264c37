"""A statement of zke_scan_signatures / zke_select_keys from OUTSIDE the engine — test infrastructure.

Scan (helpers/src/generator.rs:17-30): the oracle's exported header split (zko_parse_headers) and MIME subpart walk
(zko_mime_walk) stand for mailparse::parse_mail; the plain serial tag-list parser of tests/test_taglist_model.py (`serial`)
stands for cfdkim's parser::tag_list; validate_header's rules are written out below: the seven required tags, v=1, the i=
suffix test (or, under i_must_be_subdomain, the subdomain test), h= names "from", q= is dns/txt, and x= under enforce_expiry_x.

Selection (generator.rs:31-45): the oracle's verify_email once per (e-mail, candidate key); the first ZKE_OK wins.
"""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional, Sequence, Tuple

from zkemail_rs_amd import _abi as A

import oracle_lib
from test_taglist_model import NON_ASCII, SYNTAX, TOO_LONG, TOO_MANY, serial

REQUIRED = (b"v", b"a", b"b", b"bh", b"d", b"h", b"s")
ALGOS = {b"rsa-sha256": A.SIG_ALGO_RSA_SHA256, b"rsa-sha1": A.SIG_ALGO_RSA_SHA1, b"ed25519-sha256": A.SIG_ALGO_ED25519_SHA256}
KELVIN = "\u212a".encode("utf-8")
STRICT_EXPIRY_X, STRICT_I_SUBDOMAIN = 1, 8          # ZKE_STRICT_* (include/zkemail_amd.h)
I64_MAX = 2 ** 63 - 1


class Sig(NamedTuple):
    header_index: int
    code: int
    algo: int
    selector: bytes
    value_span: Tuple[int, int]


class Scan(NamedTuple):
    status: int
    detail: int
    sigs: List[Sig]
    n_signatures: int
    n_candidates: int


def parse_i64(s: bytes) -> int:
    """str::parse::<i64>: optional sign, ASCII digits, no overflow; anything else counts as 0 (cloudflare/dkim's x= rule)."""
    body = s[1:] if s[:1] in (b"+", b"-") else s
    if not body or any(not 0x30 <= c <= 0x39 for c in body):
        return 0
    v = int(body) * (-1 if s[:1] == b"-" else 1)
    return v if -2 ** 63 <= v <= I64_MAX else 0


def validate_header(v: bytes, strict: int = 0, now: int = 0):
    """cfdkim validate_header over a header value -> (ZKE_D_* or 0, tags by name or None)."""
    err, tags = serial(v)
    if err is not None:
        return {NON_ASCII: A.D_U_SIG_NON_ASCII, SYNTAX: A.D_SIG_SYNTAX, TOO_MANY: A.D_U_TOO_MANY_TAGS, TOO_LONG: A.D_U_SIG_TOO_LONG}[err], None
    t = {}
    for name, _, _, val in tags:
        t[name] = val                                   # the last tag of a name wins (IndexMap::insert)
    if any(r not in t for r in REQUIRED):
        return A.D_MISSING_TAG, None
    if t[b"v"] != b"1":
        return A.D_INCOMPATIBLE_VERSION, None
    if b"i" in t:
        ident, d = t[b"i"], t[b"d"]
        if strict & STRICT_I_SUBDOMAIN:
            dom = ident[ident.rfind(b"@") + 1:].lower()
            dl = d.lower()
            if not (dom == dl or (len(dom) > len(dl) and dom.endswith(dl) and dom[len(dom) - len(dl) - 1:len(dom) - len(dl)] == b".")):
                return A.D_DOMAIN_MISMATCH, None
        elif not ident.endswith(d):
            return A.D_DOMAIN_MISMATCH, None
    if not any(x.lower() == b"from" for x in t[b"h"].split(b":")):
        return A.D_FROM_NOT_SIGNED, None
    if b"q" in t and t[b"q"] != b"dns/txt":
        return A.D_BAD_QUERY_METHOD, None
    if (strict & STRICT_EXPIRY_X) and b"x" in t:
        if now > min(parse_i64(t[b"x"]) + 900, I64_MAX):
            return A.D_SIG_EXPIRED, None
    return 0, t


def split(raw: bytes):
    """mailparse::parse_mail as the oracle restates it -> (status, detail, [(key_start, key_end, val_start, val_end)])."""
    lib = oracle_lib.load().lib
    spans = (C.c_uint32 * (4 * A.MAX_HEADERS))()
    body = C.c_size_t()
    n = lib.zko_parse_headers(bytes(raw) if raw else b"\0", len(raw), C.addressof(spans), A.MAX_HEADERS, C.byref(body))
    if n < 0:
        return (A.ZKE_UNSUPPORTED if -n == A.D_U_TOO_MANY_HEADERS else A.ZKE_PARSE_FAIL), int(-n), []
    st, det = oracle_lib.load().mime_walk(raw)
    if st:
        return st, det, []
    return A.ZKE_OK, 0, [tuple(spans[4 * i:4 * i + 4]) for i in range(n)]


def scan_email(raw: bytes, from_domain: str, max_sigs: int = 8, strict: int = 0, now: int = 0) -> Scan:
    st, det, hdrs = split(raw)
    if st:
        return Scan(st, det, [], 0, 0)
    dom = from_domain.encode("utf-8")
    if KELVIN in dom:          # to_lowercase() of U+212A is ASCII "k": the engine folds ASCII only and reports the e-mail
        return Scan(A.ZKE_UNSUPPORTED, A.D_U_DOMAIN_FOLD, [], 0, 0)
    sigs: List[Sig] = []
    n_sig = n_cand = 0
    for hx, (ks, ke, vs, ve) in enumerate(hdrs):
        if raw[ks:ke].lower() != b"dkim-signature":
            continue
        code, t = validate_header(raw[vs:ve], strict, now)
        algo, sel = 0, b""
        if code == 0:
            if t[b"d"].lower() == dom.lower():          # bytes.lower(): ASCII only, as the engine folds
                n_cand += 1
            else:
                code = A.D_NEUTRAL
            algo, sel = ALGOS.get(t[b"a"], A.SIG_ALGO_OTHER), t[b"s"]
        if n_sig < max_sigs:
            sigs.append(Sig(hx, code, algo, sel, (vs, ve)))
        n_sig += 1
    return Scan(A.ZKE_OK, 0, sigs, n_sig, n_cand)


def scan(raw_emails: Sequence[bytes], from_domains: Sequence[str], max_sigs: int = 8, strict: int = 0, now: int = 0) -> List[Scan]:
    return [scan_email(r, d, max_sigs, strict, now) for r, d in zip(raw_emails, from_domains)]


def select_keys(emails: Sequence["A.Email"], candidate_keys: Sequence[Sequence[Optional["A.PublicKey"]]], threads: int = 4, **strict):
    """-> (records, chosen) as zke_select_keys defines them, from the oracle's verify_email per (e-mail, candidate key)."""
    import numpy as np
    flat = [A.Email(e.from_domain, e.raw_email, k if k is not None else A.PublicKey(b""), e.external_inputs)
            for e, ks in zip(emails, candidate_keys) for k in ks]
    recs = oracle_lib.load().verify_batch(A.PackedBatch(flat), threads=threads, **strict) if flat else np.zeros(0, A.RESULT_DTYPE)
    out = np.zeros(len(emails), A.RESULT_DTYPE)
    chosen = np.zeros(len(emails), np.uint32)
    pos = 0
    for i, ks in enumerate(candidate_keys):
        mine = recs[pos:pos + len(ks)]
        pos += len(ks)
        if not len(ks):
            out[i]["status"], out[i]["detail"] = A.ZKE_DKIM_NOT_PASS, A.D_NEUTRAL
            chosen[i] = A.SEL_NONE
            continue
        ok = [k for k in range(len(ks)) if int(mine[k]["status"]) == A.ZKE_OK]
        if not ok:
            out[i], chosen[i] = mine[-1], A.SEL_NONE
            continue
        k = ok[0]
        flag = A.SEL_AFTER_UNSUPPORTED if any(int(r["status"]) == A.ZKE_UNSUPPORTED for r in mine[:k]) else 0
        out[i], chosen[i] = mine[k], k | flag
    return out, chosen
