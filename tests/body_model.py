"""A Python statement of `extract_email_body(&parse_mail(raw).unwrap())` (core/src/email.rs:7-23) as include/zkemail_amd.h
reads it, rule by rule (1-9 there), written with string operations and the standard library: bytes.split / strip / lower,
base64.b64decode(validate=True) on the cleaned text.  Built on tests/mime_model.py (header split, get_value, parse_content_type,
the boundary-line search), which it imports and does not change; it shares nothing with the device code.

Like the MIME walk this is restated from recollection of mailparse 0.15.0, data-encoding and quoted_printable (parity unpinned,
DESIGN.md §4).  Where the engine reports ZKE_UNSUPPORTED the model raises `Undecided` (with the detail the engine names), in the
order the engine meets the cases: parts in file order, a part's own Content-Type before its subparts.
"""
from __future__ import annotations

import base64
from typing import List, NamedTuple, Optional, Tuple

from mime_model import RUST_WS, MailParseError, Undecided, find_line_prefix, get_value, parse_content_type, parse_headers

CTE_IDENTITY, CTE_BASE64, CTE_QP = 0, 1, 2
PART_HTML = 0x80000000
MAX_DEPTH = 8
# detail codes (include/zkemail_amd.h), spelled out here so that the model depends on nothing but the header's text
D_U_MIME_CTYPE, D_U_MIME_BOUNDARY, D_U_MIME_DEPTH = 67, 68, 69
D_BODY_B64_CHAR, D_BODY_B64_LENGTH, D_BODY_B64_TRAILING_BITS, D_U_BODY_CTE = 110, 111, 112, 113

B64_ALPHABET = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"
HEX = b"0123456789abcdefABCDEF"


class BodyDecodeError(Exception):
    """get_body_raw().unwrap() panics: the base64 rule the body breaks."""

    def __init__(self, detail: int):
        super().__init__(detail)
        self.detail = detail


def undecided(detail: int, why: str) -> Undecided:
    e = Undecided(why)
    e.detail = detail
    return e


def undecidable(v: bytes) -> bool:
    return any(b >= 0x80 for b in v) or b"=?" in v


# ------------------------------------------------------------------ rules 1-5: the parts
class Part(NamedTuple):
    start: int                  # the part is raw[start:end]
    end: int
    headers: List[Tuple[bytes, bytes]]
    body: int                   # where its body starts
    first_boundary: Optional[int]   # a multipart whose first boundary line was found: where that line starts
    children: list              # [Part]


def first_header(headers, name: bytes) -> Optional[bytes]:
    for k, v in headers:
        if len(k) == len(name) and k.lower() == name:
            return v
    return None


def walk(raw: bytes, start: int, end: int, level: int, open_frames: int) -> Part:
    """parse_mail_recursive over raw[start:end], with the engine's carve-outs in the engine's order."""
    data = raw[start:end]
    headers, ix_body = parse_headers(data, level)
    me = Part(start, end, headers, start + ix_body, None, [])
    ctype = first_header(headers, b"content-type")
    if ctype is None:
        return me
    token = ctype.split(b";", 1)[0]
    if undecidable(token):
        raise undecided(D_U_MIME_CTYPE, "first token of a Content-Type")
    if not get_value(token).strip(RUST_WS).lower().startswith("multipart/"):
        return me
    if undecidable(ctype):
        raise undecided(D_U_MIME_CTYPE, "multipart Content-Type")
    try:
        _, raw_params = parse_content_type(ctype.decode("ascii"))         # the parameter as it lies in the header, folds and all
    except Undecided:
        raise undecided(D_U_MIME_BOUNDARY, "RFC 2231 boundary")
    if "boundary" not in raw_params:
        return me
    if "\n" in raw_params["boundary"]:
        raise undecided(D_U_MIME_BOUNDARY, "boundary value across lines")
    if not len(data) > ix_body:
        return me
    if open_frames >= MAX_DEPTH:
        raise undecided(D_U_MIME_DEPTH, "more than 8 nested multiparts")
    _, params = parse_content_type(get_value(ctype))
    boundary = ("--" + params["boundary"]).encode("ascii")
    ix_end = find_line_prefix(data, ix_body, boundary)
    if ix_end is None:
        return me
    me = me._replace(first_boundary=start + ix_end)
    ix_boundary_end = ix_end + len(boundary)
    while True:
        nl = data.find(b"\n", ix_boundary_end)
        if nl < 0:
            break
        ps = nl + 1
        pe = find_line_prefix(data, ps, boundary)
        if pe is None:
            break                                        # no line ends this part: it is not one
        me.children.append(walk(raw, start + ps, start + pe, level + 1, open_frames + 1))
        ix_boundary_end = pe + len(boundary)
        if data[ix_boundary_end:ix_boundary_end + 2] == b"--":
            break
    return me


def mimetype(part: Part) -> str:
    v = first_header(part.headers, b"content-type")
    if v is None:
        return "text/plain"
    return get_value(v.split(b";", 1)[0]).strip(RUST_WS).lower()


def select(top: Part) -> Tuple[Part, int]:
    """(the chosen part, zke_body_info.part)"""
    for k, c in enumerate(top.children):
        if mimetype(c) == "text/html":
            return c, (k + 1) | PART_HTML
    if top.children:
        return top.children[0], 1
    return top, 0


def body_span(raw: bytes, p: Part, is_child: bool, part_keeps_eol: bool) -> Tuple[int, int]:
    start = min(p.body, p.end)
    end = p.first_boundary if p.first_boundary is not None else p.end
    # strictness site part_keeps_eol: an end that is a boundary line loses the line break in front of that line
    if (p.first_boundary is not None or is_child) and not part_keeps_eol:
        if end > start and raw[end - 1:end] == b"\n":
            end -= 1
            if end > start and raw[end - 1:end] == b"\r":
                end -= 1
    return start, end


# ------------------------------------------------------------------ rule 6: the transfer encoding
def transfer_encoding(p: Part) -> int:
    v = first_header(p.headers, b"content-transfer-encoding")
    if v is None:
        return CTE_IDENTITY
    if undecidable(v):
        raise undecided(D_U_BODY_CTE, "Content-Transfer-Encoding")
    name = get_value(v).lower()
    return {"base64": CTE_BASE64, "quoted-printable": CTE_QP}.get(name, CTE_IDENTITY)


# ------------------------------------------------------------------ rule 8: base64
def decode_base64(body: bytes) -> bytes:
    text = body
    for ws in (b"\t", b"\n", b"\x0c", b"\r", b" "):      # u8::is_ascii_whitespace; not \v
        text = text.replace(ws, b"")
    pad = 2 if text.endswith(b"==") else 1 if text.endswith(b"=") else 0
    data = text[:len(text) - pad]
    if any(c not in B64_ALPHABET for c in data):
        raise BodyDecodeError(D_BODY_B64_CHAR)
    if len(text) % 4:
        raise BodyDecodeError(D_BODY_B64_LENGTH)
    if pad:
        last = B64_ALPHABET.index(data[-1:])
        if last & (15 if pad == 2 else 3):
            raise BodyDecodeError(D_BODY_B64_TRAILING_BITS)
    return base64.b64decode(text, validate=True)


# ------------------------------------------------------------------ rule 9: quoted-printable, Robust
def decode_qp(body: bytes) -> bytes:
    kept = bytes(b for b in body if b in (9, 13, 10) or 0x20 <= b <= 0x7E)            # (a)
    pieces = kept.split(b"\n")                                                          # (b) str::lines()
    if pieces[-1] == b"":
        pieces.pop()
    out = []
    for n, piece in enumerate(pieces):
        if piece.endswith(b"\r"):
            piece = piece[:-1]
        line = piece.rstrip(b" \t\r")                                                   # (c)
        soft = False
        dec = bytearray()
        i = 0
        while i < len(line):
            if line[i:i + 1] != b"=":
                dec += line[i:i + 1]
                i += 1
                continue
            rest = line[i + 1:i + 3]
            if len(rest) == 0:                                                          # (d)
                soft = True
                i += 1
            elif len(rest) == 1:                                                        # (e)
                dec += b"=" + rest
                i += 2
            elif rest[0] in HEX and rest[1] in HEX:                                     # (f)
                dec.append(int(rest.decode("ascii"), 16))
                i += 3
            else:                                                                       # (g)
                dec += b"=" + rest
                i += 3
        out.append(bytes(dec))
        if not soft and n + 1 < len(pieces):                                            # (h)
            out.append(b"\r\n")
    return b"".join(out)


# ------------------------------------------------------------------ the call
class Body(NamedTuple):
    part: int
    encoding: int
    src_off: int
    src_len: int
    data: bytes


def locate(raw: bytes, part_keeps_eol: bool = False) -> Tuple[int, int, int, int]:
    """(part, encoding, src_off, src_len) — rules 1-6.  Raises MailParseError / Undecided."""
    top = walk(raw, 0, len(raw), 0, 0)
    p, partno = select(top)
    enc = transfer_encoding(p)
    s, e = body_span(raw, p, partno != 0, part_keeps_eol)
    return partno, enc, s, e - s


def extract(raw: bytes, part_keeps_eol: bool = False) -> Body:
    """Raises MailParseError (email.rs:26), Undecided (the engine's ZKE_UNSUPPORTED) or BodyDecodeError (email.rs:17-21)."""
    partno, enc, s, n = locate(raw, part_keeps_eol)
    src = raw[s:s + n]
    data = decode_base64(src) if enc == CTE_BASE64 else decode_qp(src) if enc == CTE_QP else src
    return Body(partno, enc, s, n, data)


def verdict(raw: bytes, part_keeps_eol: bool = False):
    """("ok", Body) | ("fail", what, depth) | ("undecided", detail) | ("decode", detail, part, encoding, src_off, src_len)"""
    try:
        return ("ok", extract(raw, part_keeps_eol))
    except MailParseError as e:
        return ("fail", e.what, e.depth)
    except Undecided as e:
        return ("undecided", getattr(e, "detail", D_U_MIME_CTYPE))
    except BodyDecodeError as e:
        return ("decode", e.detail) + locate(raw, part_keeps_eol)
