"""A statement of zke_decode_key_records from OUTSIDE the engine — test infrastructure, plain Python.

ARCHIVE (mode 0) restates helpers/src/dkim.rs:67-111: the entry filter (:69-71), the fold over value.split(';').map(str::trim)
(:74-85), the "rsa" default (:88-90), "No public key found" (:92-94), base64 0.22 STANDARD (:97, :104), from_public_key_der then
from_pkcs1_der and RsaPublicKey::new's range (:98-99; rsa 0.9.6), the 32 bytes of an Ed25519 key (:105-107), "Unsupported key
type" (:110).  str::trim is restated for its ASCII share; where Unicode white space could make a difference the answer is
D_KEYREC_NON_ASCII_EDGE ("cannot answer").

DNS (mode 1) is the TXT record of RFC 6376 3.6.1 in the tag-list grammar of the signature parser (cfdkim parser::tag_list as
tests/test_taglist_model.py states it: the last tag of a name wins, what follows the last well-formed tag-spec is not read).

to_pkcs1_der (:100): DER has one encoding per value, so the PKCS#1 bytes of a key that decoded ARE the slice it was decoded
from; the model returns that slice (tests/test_keyrec_model.py checks it against openssl's re-encoding for every fixture key).
"""
from __future__ import annotations

import re
from typing import List, NamedTuple, Optional, Sequence, Tuple

from zkemail_rs_amd import _abi as A

ARCHIVE, DNS = 0, 1
MAX_BYTES = 4096
TRIM = b"\t\n\x0b\x0c\r "                      # str::trim, ASCII share (U+0009..U+000D, U+0020)
FWS = b" \t\r\n"
B64 = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"
RSA_ALGORITHM = bytes.fromhex("300d06092a864886f70d0101010500")      # SEQUENCE { OID 1.2.840.113549.1.1.1, NULL }


class Key(NamedTuple):
    code: int                 # 0 | D_KEYREC_*
    key_type: int             # KEY_RSA / KEY_ED25519 as far as the record got, KEY_OTHER with D_KEYREC_TYPE
    key: bytes                # PKCS#1 DER or 32 raw bytes; b"" unless code is 0


def b64_standard(t: bytes) -> Optional[bytes]:
    """base64 0.22 STANDARD.decode: padding required, trailing bits zero, nothing but the alphabet.  None: an error."""
    if len(t) % 4:
        return None
    pad = 0
    if t[-1:] == b"=":
        pad = 2 if t[-2:-1] == b"=" else 1
    body = t[:len(t) - pad]
    vals = []
    for c in body:
        v = B64.find(bytes([c]))
        if v < 0:
            return None
        vals.append(v)
    if pad == 2 and vals[-1] & 15:
        return None
    if pad == 1 and vals[-1] & 3:
        return None
    bits = 0
    for v in vals:
        bits = (bits << 6) | v
    nbits = 6 * len(vals)
    nbytes = nbits // 8
    return (bits >> (nbits - 8 * nbytes)).to_bytes(nbytes, "big") if nbytes else b""


def der_tlv(b: bytes, p: int, end: int) -> Optional[Tuple[int, int, int]]:
    """One DER TLV at b[p:end] -> (tag, value start, value end): definite length in its shortest form."""
    if end - p < 2:
        return None
    tag, l0 = b[p], b[p + 1]
    q = p + 2
    if l0 < 0x80:
        ln = l0
    else:
        nb = l0 & 0x7F
        if nb == 0 or nb > 4 or q + nb > end:
            return None
        ln = int.from_bytes(b[q:q + nb], "big")
        if b[q] == 0 or (nb == 1 and ln < 0x80) or ln >= 2 ** 31:
            return None
        q += nb
    if q + ln > end:
        return None
    return tag, q, q + ln


def der_uint(b: bytes, p: int, end: int) -> Optional[Tuple[int, int]]:
    """A non-negative INTEGER in its shortest form -> (value, position behind it)."""
    t = der_tlv(b, p, end)
    if t is None or t[0] != 0x02 or t[2] == t[1]:
        return None
    v = b[t[1]:t[2]]
    if v[0] & 0x80 or (len(v) > 1 and v[0] == 0 and not v[1] & 0x80):
        return None
    return int.from_bytes(v, "big"), t[2]


def pkcs1(b: bytes) -> int:
    """RSAPublicKey ::= SEQUENCE { modulus INTEGER, publicExponent INTEGER } filling b, then RsaPublicKey::new's range."""
    t = der_tlv(b, 0, len(b))
    if t is None or t[0] != 0x30 or t[2] != len(b):
        return A.D_KEYREC_DER
    n = der_uint(b, t[1], t[2])
    if n is None:
        return A.D_KEYREC_DER
    e = der_uint(b, n[1], t[2])
    if e is None or e[1] != t[2]:
        return A.D_KEYREC_DER
    if n[0].bit_length() > 4096 or not 2 <= e[0] <= 2 ** 33 - 1:
        return A.D_KEYREC_RANGE
    return 0


def spki(b: bytes) -> Tuple[int, bytes]:
    """SubjectPublicKeyInfo filling b: rsaEncryption with a NULL parameter, BIT STRING with 0 unused bits -> (code, PKCS#1 slice)."""
    t = der_tlv(b, 0, len(b))
    if t is None or t[0] != 0x30 or t[2] != len(b):
        return A.D_KEYREC_DER, b""
    p = t[1]
    if b[p:p + 15] != RSA_ALGORITHM:
        return A.D_KEYREC_DER, b""
    bs = der_tlv(b, p + 15, t[2])
    if bs is None or bs[0] != 0x03 or bs[2] != t[2] or bs[2] - bs[1] < 1 or b[bs[1]] != 0:
        return A.D_KEYREC_DER, b""
    inner = b[bs[1] + 1:bs[2]]
    return pkcs1(inner), inner


def rsa_key(der: bytes) -> Tuple[int, bytes]:
    code, inner = spki(der)                    # from_public_key_der ...
    if code == 0:
        return 0, inner
    if code == A.D_KEYREC_RANGE:               # (a SubjectPublicKeyInfo is no RSAPublicKey: its first member is a SEQUENCE)
        return code, b""
    code = pkcs1(der)                          # ... .or_else(from_pkcs1_der)
    return code, der if code == 0 else b""


def archive_tags(v: bytes):
    """dkim.rs:69-94 -> (code, key type text, key text)."""
    if b"p=" not in v or v.endswith(b"p="):
        return A.D_KEYREC_NO_KEY, b"", b""
    kt = pk = b""
    edge = False
    for part in v.split(b";"):
        t = part.strip(TRIM)
        if t and (t[0] >= 0x80 or t[-1] >= 0x80):
            edge = True
        if t.startswith(b"k="):
            kt = t[2:]
        if t.startswith(b"p="):
            pk = t[2:]
    if edge:
        return A.D_KEYREC_NON_ASCII_EDGE, b"", b""
    return 0, kt, pk


TAG_SPEC = re.compile(rb"[ \t\r\n]*([A-Za-z][A-Za-z0-9_]*)[ \t\r\n]*=([\x21-\x3a\x3c-\x7e \t\r\n]*)")


def dns_tags(v: bytes):
    """RFC 6376 3.6.1 over the signature parser's tag-list grammar -> (code, key type text, key text), FWS removed."""
    if any(c >= 0x80 for c in v):
        return A.D_KEYREC_SYNTAX, b"", b""
    kt, pk = b"", None
    pos = idx = 0
    while True:
        m = TAG_SPEC.match(v, pos)
        if m is None:
            if idx == 0:
                return A.D_KEYREC_SYNTAX, b"", b""
            break
        name, val = m.group(1), bytes(c for c in m.group(2) if c not in FWS)
        if name == b"v" and (idx != 0 or val != b"DKIM1"):
            return A.D_KEYREC_VERSION, b"", b""
        if name == b"k":
            kt = val
        if name == b"p":
            pk = val
        idx += 1
        if v[m.end():m.end() + 1] != b";":
            break
        pos = m.end() + 1
    if pk is None:
        return A.D_KEYREC_NO_KEY, b"", b""
    return 0, kt, pk


def decode(record: bytes, mode: int = ARCHIVE) -> Key:
    if len(record) == 0:                               # the fetch failed (generator.rs:33)
        return Key(A.D_KEYREC_NO_KEY, 0, b"")
    if len(record) > MAX_BYTES:
        return Key(A.D_KEYREC_TOO_LONG, 0, b"")
    code, kt, pk = (archive_tags if mode == ARCHIVE else dns_tags)(record)
    if code:
        return Key(code, 0, b"")
    if not pk:
        return Key(A.D_KEYREC_NO_KEY, 0, b"")
    if kt in (b"", b"rsa"):
        ktype = A.KEY_RSA
    elif kt == b"ed25519":
        ktype = A.KEY_ED25519
    else:
        return Key(A.D_KEYREC_TYPE, A.KEY_OTHER, b"")
    raw = b64_standard(pk)
    if raw is None:
        return Key(A.D_KEYREC_B64, ktype, b"")
    if ktype == A.KEY_ED25519:
        return Key(0, ktype, raw) if len(raw) == 32 else Key(A.D_KEYREC_ED25519_LEN, ktype, b"")
    code, key = rsa_key(raw)
    return Key(code, ktype, key)


def decode_all(records: Sequence[bytes], mode: int = ARCHIVE) -> List[Key]:
    return [decode(r, mode) for r in records]


def public_key(k: Key) -> "A.PublicKey":
    """The candidate zke_select_keys takes for a decoded record: a record without a key is an empty RSA key."""
    return A.PublicKey(k.key, "ed25519" if k.code == 0 and k.key_type == A.KEY_ED25519 else "rsa")
