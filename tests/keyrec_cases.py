"""Inputs of the key-record tests (tests/test_keyrec_model.py, tests/test_gpu_keyrec.py): the fixture keys as records, the
hand-written cases with the code each rule gives — written down here, not asked of the model —, and the seeded mutation fuzz.
Nothing here asks the engine for anything."""
from __future__ import annotations

import base64
import json
import os
from typing import List, Tuple

import numpy as np

from zkemail_rs_amd import _abi as A

import synth

ARCHIVE, DNS = 0, 1
HERE = os.path.dirname(os.path.abspath(__file__))
RSA_ALGORITHM = bytes.fromhex("300d06092a864886f70d0101010500")


def b64(b: bytes) -> bytes:
    return base64.b64encode(b)


def der_len(n: int) -> bytes:
    if n < 0x80:
        return bytes([n])
    body = n.to_bytes((n.bit_length() + 7) // 8, "big")
    return bytes([0x80 | len(body)]) + body


def tlv(tag: int, body: bytes) -> bytes:
    return bytes([tag]) + der_len(len(body)) + body


def der_int(v: int) -> bytes:
    body = v.to_bytes(max(1, (v.bit_length() + 8) // 8), "big")          # a leading zero where the top bit is set
    return tlv(0x02, body)


def pkcs1_of(n: int, e: int) -> bytes:
    return tlv(0x30, der_int(n) + der_int(e))


def spki_wrap(pkcs1: bytes, algorithm: bytes = RSA_ALGORITHM, unused: int = 0) -> bytes:
    """SubjectPublicKeyInfo around a PKCS#1 key (tests/test_keyrec_model.py checks it against openssl for every fixture key)."""
    return tlv(0x30, algorithm + tlv(0x03, bytes([unused]) + pkcs1))


def rfc8463():
    with open(os.path.join(HERE, "golden", "rfc8463_appendix_a.json")) as f:
        return json.load(f)


def fixture_records() -> List[Tuple[str, bytes, int, bytes]]:
    """(name, record, key type, the key it decodes to): every RSA fixture key as SubjectPublicKeyInfo and as PKCS#1 in a handful
    of spellings, the Ed25519 fixture keys, the two records of RFC 8463 A.2."""
    out = []
    for i, (name, k) in enumerate(sorted(synth.load_keys().items())):
        sp = b64(spki_wrap(k.pkcs1_der))
        pk = b64(k.pkcs1_der)
        out.append((name + "/spki", [b"v=DKIM1; k=rsa; p=", b"p=", b"v=DKIM1;p=", b"k=rsa;t=s;p="][i % 4] + sp, A.KEY_RSA, k.pkcs1_der))
        out.append((name + "/pkcs1", [b"k=rsa; p=", b"v=DKIM1; p=", b"v=DKIM1; h=sha256; k=rsa; p="][i % 3] + pk + [b"", b";", b"; n=note"][i % 3],
                    A.KEY_RSA, k.pkcs1_der))
    for j, ed in enumerate(synth.ed_keys(4)):
        out.append((f"ed{j}", b"v=DKIM1; k=ed25519; p=" + b64(ed.pub), A.KEY_ED25519, ed.pub))
    r = rfc8463()
    out.append(("rfc8463/rsa", b"v=DKIM1; k=rsa; p=" + r["rsa"]["p_base64_spki"].encode(), A.KEY_RSA, None))
    out.append(("rfc8463/ed25519", b"v=DKIM1; k=ed25519; p=" + r["ed25519"]["p_base64"].encode(), A.KEY_ED25519,
                base64.b64decode(r["ed25519"]["p_base64"])))
    return out


def hand_cases():
    """(name, mode, record, code, key type, key or b"") — the code is what the rule named in `name` gives, by hand."""
    k = synth.load_keys()
    k1, k2 = k["rsa1024_00"], k["rsa2048_00"]
    p1, p2 = k1.pkcs1_der, k2.pkcs1_der
    s1 = spki_wrap(p1)
    ed = synth.ed_keys(1)[0].pub
    R, E, O = A.KEY_RSA, A.KEY_ED25519, A.KEY_OTHER
    AR, DN = ARCHIVE, DNS
    big_n = (1 << 4096) | k2.n                                        # 4097 bits
    body1 = der_int(k1.n) + der_int(k1.e)                             # 137 bytes: its length needs one octet behind 0x81
    assert len(body1) < 256 and b64(ed).endswith(b"=") and b64(ed[:31]).endswith(b"==")
    c = [
        # ---- ARCHIVE: dkim.rs:67-111
        ("last p= wins", AR, b"p=" + b64(p1) + b"; p=" + b64(p2), 0, R, p2),
        ("last k= wins", AR, b"k=ed25519; k=rsa; p=" + b64(s1), 0, R, p1),
        ("last k= wins (ed25519)", AR, b"k=rsa; p=" + b64(ed) + b"; k=ed25519", 0, E, ed),
        ("an empty last k= is rsa", AR, b"k=ed25519; k=; p=" + b64(p1), 0, R, p1),
        ("K= is not a tag", AR, b"K=ed25519; p=" + b64(p1), 0, R, p1),
        ("P= is not a tag", AR, b"p=" + b64(p1) + b"; P=" + b64(p2), 0, R, p1),
        ("k=RSA is unsupported", AR, b"k=RSA; p=" + b64(p1), A.D_KEYREC_TYPE, O, b""),
        ("k= rsa keeps its blank", AR, b"k= rsa; p=" + b64(p1), A.D_KEYREC_TYPE, O, b""),
        ("p= x", AR, b"v=DKIM1; p= x", A.D_KEYREC_B64, R, b""),
        ("a blank inside p=", AR, b"p= " + b64(p1), A.D_KEYREC_B64, R, b""),
        ("the record ends with p=", AR, b"v=DKIM1; k=rsa; p=", A.D_KEYREC_NO_KEY, 0, b""),
        ("no p= at all", AR, b"v=DKIM1; k=rsa", A.D_KEYREC_NO_KEY, 0, b""),
        ("p= empty in the middle, p= elsewhere", AR, b"p=; x=p=1", A.D_KEYREC_NO_KEY, 0, b""),
        ("the filter sees p= anywhere, the fold does not", AR, b"xp=" + b64(p1), A.D_KEYREC_NO_KEY, 0, b""),
        ("an empty record", AR, b"", A.D_KEYREC_NO_KEY, 0, b""),
        ("parts are trimmed, ASCII set", AR, b"\x0b\x0c k=rsa \t;\r\n p=" + b64(p1) + b" \n", 0, R, p1),
        ("unpadded base64", AR, b"k=ed25519; p=" + b64(ed).rstrip(b"="), A.D_KEYREC_B64, E, b""),
        ("padding inside", AR, b"p=AA==" + b64(p1), A.D_KEYREC_B64, R, b""),
        ("non-zero trailing bits, one pad", AR, b"k=ed25519; p=" + b64(ed)[:-2] + b"F=", A.D_KEYREC_B64, E, b""),
        ("non-zero trailing bits, two pads", AR, b"k=ed25519; p=" + b64(ed[:31])[:-3] + b"B==", A.D_KEYREC_B64, E, b""),
        ("white space inside base64", AR, b"p=" + b64(p1)[:40] + b" " + b64(p1)[40:], A.D_KEYREC_B64, R, b""),
        ("line break inside base64", AR, b"p=" + b64(p1)[:40] + b"\r\n" + b64(p1)[40:], A.D_KEYREC_B64, R, b""),
        ("url-safe alphabet", AR, b"p=" + b64(p1).replace(b"+", b"-").replace(b"/", b"_"), A.D_KEYREC_B64, R, b""),
        ("bytes trailing the SEQUENCE (SPKI)", AR, b"p=" + b64(s1 + b"\0"), A.D_KEYREC_DER, R, b""),
        ("bytes trailing the SEQUENCE (PKCS#1)", AR, b"p=" + b64(p1 + b"\0\0"), A.D_KEYREC_DER, R, b""),
        ("a missing NULL parameter", AR, b"p=" + b64(spki_wrap(p1, bytes.fromhex("300b06092a864886f70d010101"))), A.D_KEYREC_DER, R, b""),
        ("a wrong OID", AR, b"p=" + b64(spki_wrap(p1, bytes.fromhex("300d06092a864886f70d01010b0500"))), A.D_KEYREC_DER, R, b""),
        ("unused bits != 0", AR, b"p=" + b64(spki_wrap(p1, unused=1)), A.D_KEYREC_DER, R, b""),
        ("a non-minimal length", AR, b"p=" + b64(b"\x30\x82" + len(body1).to_bytes(2, "big") + body1), A.D_KEYREC_DER, R, b""),
        ("a non-minimal integer", AR, b"p=" + b64(tlv(0x30, der_int(k1.n) + b"\x02\x04\x00\x01\x00\x01")), A.D_KEYREC_DER, R, b""),
        ("a negative modulus", AR, b"p=" + b64(tlv(0x30, tlv(0x02, k1.n.to_bytes(128, "big")) + der_int(65537))), A.D_KEYREC_DER, R, b""),
        ("garbage", AR, b"p=" + b64(bytes(range(200))), A.D_KEYREC_DER, R, b""),
        ("a 4096-bit modulus", AR, b"p=" + b64(spki_wrap(k["rsa4096_00"].pkcs1_der)), 0, R, k["rsa4096_00"].pkcs1_der),
        ("a 4097-bit modulus", AR, b"p=" + b64(pkcs1_of(big_n, 65537)), A.D_KEYREC_RANGE, R, b""),
        ("a 4097-bit modulus in SPKI", AR, b"p=" + b64(spki_wrap(pkcs1_of(big_n, 65537))), A.D_KEYREC_RANGE, R, b""),
        ("e = 1", AR, b"p=" + b64(pkcs1_of(k1.n, 1)), A.D_KEYREC_RANGE, R, b""),
        ("e = 2", AR, b"p=" + b64(pkcs1_of(k1.n, 2)), 0, R, pkcs1_of(k1.n, 2)),
        ("e = 2^33 - 1", AR, b"p=" + b64(spki_wrap(pkcs1_of(k1.n, 2 ** 33 - 1))), 0, R, pkcs1_of(k1.n, 2 ** 33 - 1)),
        ("e = 2^33", AR, b"p=" + b64(pkcs1_of(k1.n, 2 ** 33)), A.D_KEYREC_RANGE, R, b""),
        ("e of nine bytes", AR, b"p=" + b64(spki_wrap(pkcs1_of(k1.n, 2 ** 64 + 1))), A.D_KEYREC_RANGE, R, b""),
        ("a 31-byte Ed25519 key", AR, b"k=ed25519; p=" + b64(ed[:31]), A.D_KEYREC_ED25519_LEN, E, b""),
        ("a 33-byte Ed25519 key", AR, b"k=ed25519; p=" + b64(ed + b"\x01"), A.D_KEYREC_ED25519_LEN, E, b""),
        ("an Ed25519 key under k=rsa", AR, b"k=rsa; p=" + b64(ed), A.D_KEYREC_DER, R, b""),
        ("k=dsa", AR, b"k=dsa; p=" + b64(p1), A.D_KEYREC_TYPE, O, b""),
        ("the type is looked at before the base64", AR, b"k=x; p=!!!", A.D_KEYREC_TYPE, O, b""),
        ("a non-ASCII edge in front", AR, b"\xc2\xa0k=rsa; p=" + b64(p1), A.D_KEYREC_NON_ASCII_EDGE, 0, b""),
        ("a non-ASCII edge behind p=", AR, b"k=rsa; p=" + b64(p1) + b"\xc2\xa0", A.D_KEYREC_NON_ASCII_EDGE, 0, b""),
        ("a part of Unicode white space only", AR, b"p=" + b64(p1) + b"; \xe3\x80\x80 ", A.D_KEYREC_NON_ASCII_EDGE, 0, b""),
        ("non-ASCII inside a part is an ordinary byte", AR, b"n=caf\xc3\xa9 au lait; p=" + b64(p1), 0, R, p1),
        ("non-ASCII inside p= is bad base64", AR, b"p=AA\xc3\xa9AAA==", A.D_KEYREC_B64, R, b""),
        ("FWS is not removed in this mode", AR, b"v=DKIM1; p=" + b64(p1)[:60] + b"\r\n\t" + b64(p1)[60:], A.D_KEYREC_B64, R, b""),
        ("v= is not looked at in this mode", AR, b"p=" + b64(p1) + b"; v=DKIM2", 0, R, p1),
        # ---- DNS: RFC 6376 3.6.1
        ("FWS inside p=", DN, b"v=DKIM1; k=rsa;\r\n\tp=" + b64(s1)[:50] + b"\r\n " + b64(s1)[50:100] + b" \t" + b64(s1)[100:], 0, R, p1),
        ("FWS around names and values", DN, b" v = DKIM1 ;\r\n k\t=\trsa ; p = " + b64(p1) + b" ; ", 0, R, p1),
        ("FWS inside k=", DN, b"k=ed2\r\n 5519; p=" + b64(ed), 0, E, ed),
        ("v= not first", DN, b"k=rsa; v=DKIM1; p=" + b64(p1), A.D_KEYREC_VERSION, 0, b""),
        ("v=DKIM2", DN, b"v=DKIM2; p=" + b64(p1), A.D_KEYREC_VERSION, 0, b""),
        ("v=dkim1", DN, b"v=dkim1; p=" + b64(p1), A.D_KEYREC_VERSION, 0, b""),
        ("v= twice", DN, b"v=DKIM1; v=DKIM1; p=" + b64(p1), A.D_KEYREC_VERSION, 0, b""),
        ("no v=", DN, b"p=" + b64(p1), 0, R, p1),
        ("an empty p= (revoked)", DN, b"v=DKIM1; k=rsa; p=", A.D_KEYREC_NO_KEY, 0, b""),
        ("an empty p= with FWS (revoked)", DN, b"v=DKIM1; p= \r\n ; t=y", A.D_KEYREC_NO_KEY, 0, b""),
        ("no p=", DN, b"v=DKIM1; k=rsa; t=y", A.D_KEYREC_NO_KEY, 0, b""),
        ("k= absent is rsa", DN, b"v=DKIM1; p=" + b64(s1), 0, R, p1),
        ("h= s= t= n= are ignored", DN, b"v=DKIM1; h=sha256; s=email; t=y:s; n=a note; p=" + b64(p1), 0, R, p1),
        ("k=RSA is unsupported", DN, b"v=DKIM1; k=RSA; p=" + b64(p1), A.D_KEYREC_TYPE, O, b""),
        ("no tag-list", DN, b"=DKIM1; p=" + b64(p1), A.D_KEYREC_SYNTAX, 0, b""),
        ("a record of blanks", DN, b"  \r\n ", A.D_KEYREC_SYNTAX, 0, b""),
        ("a byte >= 0x80", DN, b"v=DKIM1; n=caf\xc3\xa9; p=" + b64(p1), A.D_KEYREC_SYNTAX, 0, b""),
        ("what follows a malformed tag-spec is not read", DN, b"v=DKIM1; k=rsa; !; p=" + b64(p1), A.D_KEYREC_NO_KEY, 0, b""),
        ("the last p= wins", DN, b"p=" + b64(p2) + b"; p=" + b64(p1), 0, R, p1),
        ("unpadded base64", DN, b"k=ed25519; p=" + b64(ed).rstrip(b"="), A.D_KEYREC_B64, E, b""),
        ("a 31-byte Ed25519 key", DN, b"v=DKIM1; k=ed25519; p=" + b64(ed[:31]), A.D_KEYREC_ED25519_LEN, E, b""),
        ("e = 1", DN, b"v=DKIM1; p=" + b64(spki_wrap(pkcs1_of(k1.n, 1))), A.D_KEYREC_RANGE, R, b""),
        ("an empty record", DN, b"", A.D_KEYREC_NO_KEY, 0, b""),
    ]
    return c


def limit_records(mode: int):
    """Records of ZKE_KEYREC_MAX_BYTES - 1, exactly that, and + 1 bytes: an RSA-4096 record padded with an ignored tag."""
    k = synth.load_keys()["rsa4096_00"]
    head = b"v=DKIM1; k=rsa; p=" + b64(spki_wrap(k.pkcs1_der)) + b"; n="
    out = []
    for total in (A.KEYREC_MAX_BYTES - 1, A.KEYREC_MAX_BYTES, A.KEYREC_MAX_BYTES + 1):
        rec = head + b"x" * (total - len(head))
        out.append((rec, A.D_KEYREC_TOO_LONG if total > A.KEYREC_MAX_BYTES else 0, k.pkcs1_der if total <= A.KEYREC_MAX_BYTES else b""))
    return out


PRINTABLE = bytes(range(0x20, 0x7f)) + b"\t\r\n"
B64_ALPHABET = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"


def fuzz_records(seed: int, count: int = 4096) -> List[bytes]:
    """Half: one character inside p= replaced by another of the base64 alphabet.  Half structural: a character deleted or inserted
    (printable ASCII, tab, CR, LF), tags reordered, duplicated or re-spelled, DER bytes changed before encoding."""
    rng = np.random.default_rng(seed)
    keys = synth.load_keys()
    rsa = [keys[n] for n in ("rsa1024_00", "rsa2048_00", "rsa2048_01", "rsa3072_00", "rsa4096_00", "rsa2048e3_00")]
    eds = synth.ed_keys(4)

    def pick(seq):
        return seq[int(rng.integers(0, len(seq)))]

    def base():
        """-> (tags as [name, value] in order, index of p)"""
        if rng.random() < 0.2:
            tags = [[b"v", b"DKIM1"], [b"k", b"ed25519"], [b"p", b64(pick(eds).pub)]]
        else:
            kk = pick(rsa)
            der = spki_wrap(kk.pkcs1_der) if rng.random() < 0.7 else kk.pkcs1_der
            tags = [[b"v", b"DKIM1"], [b"k", b"rsa"], [b"p", b64(der)]]
            if rng.random() < 0.3:
                del tags[1]
        if rng.random() < 0.3:
            tags.insert(int(rng.integers(1, len(tags))), pick([[b"t", b"s"], [b"h", b"sha256"], [b"n", b"a note"], [b"s", b"email"]]))
        return tags

    def join(tags):
        sep = pick([b"; ", b";", b" ; "])
        return sep.join(n + b"=" + v for n, v in tags) + pick([b"", b";"])

    out = []
    for i in range(count):
        tags = base()
        pi = [j for j, t in enumerate(tags) if t[0] == b"p"][0]
        if i % 2 == 0:
            v = bytearray(tags[pi][1])
            v[int(rng.integers(0, len(v)))] = pick(B64_ALPHABET)
            tags[pi][1] = bytes(v)
            out.append(join(tags))
            continue
        op = int(rng.integers(0, 6))
        if op == 0:                                   # DER bytes changed before encoding
            der = bytearray(base64.b64decode(tags[pi][1]))
            for _ in range(int(rng.integers(1, 3))):
                pos = int(rng.integers(0, min(len(der), 40))) if rng.random() < 0.7 else int(rng.integers(0, len(der)))
                der[pos] = int(rng.integers(0, 256))
            if rng.random() < 0.2:
                der = der[:-1] if rng.random() < 0.5 else der + b"\0"
            tags[pi][1] = b64(bytes(der))
            out.append(join(tags))
        elif op == 1:                                 # tags reordered
            rng.shuffle(tags)
            out.append(join(tags))
        elif op == 2:                                 # a tag duplicated, perhaps with another value
            j = int(rng.integers(0, len(tags)))
            dup = [tags[j][0], tags[j][1] if rng.random() < 0.5 else pick([b"", b"rsa", b"ed25519", b"DKIM1", b"AAAA"])]
            tags.insert(int(rng.integers(0, len(tags) + 1)), dup)
            out.append(join(tags))
        elif op == 3:                                 # a tag re-spelled
            j = int(rng.integers(0, len(tags)))
            how = int(rng.integers(0, 4))
            if how == 0:
                tags[j][0] = tags[j][0].upper()
            elif how == 1:
                tags[j][1] = tags[j][1].swapcase() if tags[j][0] != b"p" else tags[j][1].rstrip(b"=")
            elif how == 2:
                tags[j][0] = tags[j][0] + b" "
            else:
                tags[j][1] = b" " + tags[j][1]
            out.append(join(tags))
        else:                                         # a character deleted or inserted anywhere
            rec = bytearray(join(tags))
            for _ in range(int(rng.integers(1, 3))):
                pos = int(rng.integers(0, len(rec)))
                if rng.random() < 0.5:
                    del rec[pos]
                else:
                    rec.insert(pos, pick(PRINTABLE))
            out.append(bytes(rec))
    return out
