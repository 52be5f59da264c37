"""Inputs of the signature-scan and key-selection tests (tests/test_sigscan_model.py, tests/test_gpu_sigscan.py): the shared
case corpus with many-signature e-mails, the tag-list fuzz headers, MIME-fuzz and byte-mutation-fuzz e-mails, e-mails with a
given number of DKIM-Signature headers, selectors of given lengths, and the two-signature workload of the chain test.  Every
e-mail is made by the Python signer (tests/synth.py); nothing here asks the engine or the oracle for anything."""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

from zkemail_rs_amd import _abi as A

import cases
import synth
from synth import SignSpec, sign_email

Pair = Tuple[bytes, str]          # (raw e-mail, from_domain)


def corpus() -> Tuple[List[str], List[Pair], List[cases.Case]]:
    """cases.build_cases() + build_limit_cases() + e-mails with 3, 4, 6 and 21 same-domain signatures."""
    cs = cases.build_cases() + cases.build_limit_cases() + [cases.multi_signature_case(k) for k in (2, 3, 5, 20)]
    return [c.name for c in cs], [(c.email.raw_email, c.email.from_domain) for c in cs], cs


def taglist_headers(seeds=(1, 2, 3, 4), per_seed: int = 1024):
    """The 4 096 signature layouts of tests/taglist_fuzz.py as tests/test_taglist.py makes them -> (pairs, kinds, emails)."""
    import test_taglist
    pairs, kinds, emails = [], [], []
    for sd in seeds:
        ems, ks = test_taglist.make(sd, per_seed)
        pairs += [(e.raw_email, e.from_domain) for e in ems]
        kinds += ks
        emails += ems
    return pairs, kinds, emails


def mime_fuzz_emails(seeds=((11, 0.0), (12, 0.2)), per_seed: int = 768) -> List[Pair]:
    """Signed e-mails whose bodies are random multipart trees (tests/mime_fuzz.py), as the verify path's MIME fuzz builds them."""
    import mime_fuzz
    k0 = synth.load_keys()["rsa2048_00"]
    out = []
    for seed, exotic in seeds:
        rng = np.random.default_rng(seed)
        for i in range(per_seed):
            ct, body = mime_fuzz.message(rng, bad=0.12, exotic=exotic, mutate=0.25)
            hs = [(n, v) for n, v in synth.std_headers(rng, i, "example.com") if n != b"Content-Type"]
            if ct is not None:
                hs.insert(int(rng.integers(0, len(hs) + 1)), (b"Content-Type", ct))
            if rng.random() < 0.3:
                body = body + synth.ascii_body(rng, int(rng.integers(100, 6000)))
            raw, _ = sign_email(hs, body, k0, SignSpec(header_canon="relaxed", body_canon="relaxed" if i % 2 else "simple"))
            out.append((raw, "example.com"))
    return out


SPECIALS = [b"\r\n", b"\n", b"\r", b" ", b"\t", b":", b";", b"=", b"\r\n\r\n", b"\r\n ", b"", b"DKIM-Signature: v=1\r\n", b"\x80",
            b"DKIM-Signature: v=1; a=rsa-sha256; d=example.com; s=m; h=from; bh=AA==; b=AA==\r\n", b"dkim-signature:", b"d=", b"s=", b"@"]


def mutation_fuzz_emails(seed: int, count: int = 600) -> List[Pair]:
    """Byte-level mutations of valid e-mails, four in five inside the header block: a byte replaced, a special inserted, bytes
    deleted, a byte replaced by a special (line ends, tag-list punctuation, whole signature headers)."""
    rng = np.random.default_rng(seed)
    ok = [c for c in cases.build_cases() if c.status == A.ZKE_OK]
    base = [c.email for c in ok if "ed25519" not in c.name][:24] + [c.email for c in ok if "ed25519" in c.name]
    base += [cases.multi_signature_case(k).email for k in (1, 3)]
    out = []
    for _ in range(count):
        e = base[int(rng.integers(0, len(base)))]
        raw = bytearray(e.raw_email)
        hdr_end = raw.find(b"\r\n\r\n")
        for _ in range(int(rng.integers(1, 4))):
            region_end = hdr_end if rng.random() < 0.8 and hdr_end > 0 else len(raw)
            pos = int(rng.integers(0, max(region_end, 1)))
            op = rng.integers(0, 4)
            if op == 0 and len(raw):
                raw[pos] = int(rng.integers(0, 256))
            elif op == 1:
                raw[pos:pos] = SPECIALS[int(rng.integers(0, len(SPECIALS)))]
            elif op == 2 and len(raw) > 2:
                del raw[pos:pos + int(rng.integers(1, 4))]
            else:
                raw[pos:pos + 1] = SPECIALS[int(rng.integers(0, len(SPECIALS)))]
        dom = e.from_domain if rng.random() < 0.9 else [e.from_domain.upper(), "other.org", "", e.from_domain + "."][int(rng.integers(0, 4))]
        out.append((bytes(raw), dom))
    return out


def _sig_header(hs, body, key, spec) -> bytes:
    """The DKIM-Signature header field (with its CRLF) the signer puts in front of the message."""
    raw, _ = sign_email(hs, body, key, spec)
    first = hs[0][0] + b":"
    return raw[:raw.find(first)]


def email_with_signatures(n_sigs: int, seed: int = 0) -> Pair:
    """n_sigs DKIM-Signature headers in front of one message, the kinds in turn: ours (candidate), another domain's, ours with h=
    lacking from, ours with v=2, ours again under another selector; every one has a selector of its own."""
    k0, k1 = cases.K("rsa2048_00"), cases.K("rsa2048_01")
    hs, body = cases._hdrs(60 + seed), cases._body(200, 60 + seed)
    msg = b"".join(n + b": " + v + b"\r\n" for n, v in hs) + b"\r\n" + body
    sigs = b""
    for j in range(n_sigs):
        kind = (j + seed) % 5
        if kind == 0:
            s = _sig_header(hs, body, k0, SignSpec(selector=f"good{j}"))
        elif kind == 1:
            s = _sig_header(hs, body, k1, SignSpec(domain="other.org", selector=f"foreign{j}"))
        elif kind == 2:
            s = _sig_header(hs, body, k0, SignSpec(selector=f"nofrom{j}", signed=("to", "subject")))
        elif kind == 3:
            s = _sig_header(hs, body, k0, SignSpec(selector=f"v2x{j}")).replace(b"v=1;", b"v=2;", 1)
        else:
            s = _sig_header(hs, body, k1, SignSpec(selector=f"again{j}", algo="rsa-sha1"))
        sigs += s
    return sigs + msg, "example.com"


def selector_emails(lengths=(1, 63, 64, 65, 253, 2000)) -> Tuple[List[Pair], List[bytes]]:
    """One signature each, its s= value of the given length; from 200 bytes on folded over many lines (FWS is stripped from
    it).  A selector of 2 000 bytes leaves 48 bytes of the tag buffer: that header is hand-made with the shortest values
    validate_header accepts (it is a candidate for the scan; it would not verify)."""
    k0 = cases.K("rsa2048_00")
    pairs, sels = [], []
    for k, L in enumerate(lengths):
        sel = ("s" + "abcdefghij"[k % 10] * (L - 1))[:L] if L > 1 else "s"
        hs, body = cases._hdrs(70 + k), cases._body(150, 70 + k)
        folded = b"\r\n\t".join(sel.encode()[i:i + 61] for i in range(0, L, 61)) if L > 200 else sel.encode()
        if L > 1500:
            raw = b"DKIM-Signature: v=1; a=x; d=example.com; h=from; bh=B; b=A; s=" + folded + b"\r\n" + \
                  b"".join(n + b": " + v + b"\r\n" for n, v in hs) + b"\r\n" + body
        else:
            raw, _ = sign_email(hs, body, k0, SignSpec(selector=sel, fold_sig=False))
            raw = raw.replace(b"s=" + sel.encode(), b"s=" + folded, 1)
        pairs.append((raw, "example.com"))
        sels.append(sel.encode())
    return pairs, sels


def chain_workload(n: int = 1024, n_keys: int = 16, seed: int = 77, unsigned_frac: float = 0.01, body_len: int = 1500):
    """The two-signature workload: every signed e-mail carries a signature of other.org first and its own second, under one of
    n_keys keys (selector = the key's number); about one e-mail in a hundred carries no signature at all.
    -> (from_domains, raw_emails, resolver dict {(domain, selector bytes): PublicKey}, indices of the unsigned e-mails)"""
    rng = np.random.default_rng(seed)
    keys = synth.keys_of(2048, n_keys)
    foreign = synth.keys_of(2048, n_keys)[::-1]
    resolver = {("example.com", b"key%02d" % k): A.PublicKey(keys[k].pkcs1_der) for k in range(n_keys)}
    doms, raws, unsigned = [], [], []
    for i in range(n):
        k = i % n_keys
        hs = synth.std_headers(rng, i, "example.com")
        body = synth.ascii_body(rng, int(rng.integers(200, body_len)))
        if rng.random() < unsigned_frac:
            raws.append(b"".join(a + b": " + v + b"\r\n" for a, v in hs) + b"\r\n" + body)
            unsigned.append(i)
        else:
            raw, _ = sign_email(hs, body, keys[k], SignSpec(selector="key%02d" % k))
            raws.append(_sig_header(hs, body, foreign[k], SignSpec(domain="other.org", selector="o%02d" % k)) + raw)
        doms.append("example.com")
    return doms, raws, resolver, unsigned
