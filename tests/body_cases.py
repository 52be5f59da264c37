"""Inputs for the body extraction (zke_extract_bodies, tests/body_model.py): the named edge list and a seeded generator of
multipart e-mails.  W is the width of one decode step of body_extract_kernel (csrc/bodyext.hip.h: 64 bytes of the part per step;
the quoted-printable decoder looks at windows of 62 filtered characters, base64 decodes rounds of 256 cleaned characters, the
part is staged 1 024 bytes at a time) — the edges below are placed against those numbers, counted from the start of the body."""
from __future__ import annotations

import base64
import quopri
import random
from typing import List, Tuple

W = 64
QP_WIN = 62
B64_ROUND = 256
TILE = 1024


def leaf(cte: bytes | None, body: bytes, extra: bytes = b"") -> bytes:
    """A message without subparts: the body is everything behind the empty line, nothing is chopped."""
    h = b"From: a@example.com\r\nSubject: s\r\n" + extra
    if cte is not None:
        h += b"Content-Transfer-Encoding: " + cte + b"\r\n"
    return h + b"\r\n" + body


def b64_cases() -> List[Tuple[str, bytes]]:
    enc = lambda n: base64.b64encode(bytes((7 * i + 3) & 0xFF for i in range(n)))
    out = [
        ("b64_clean_0", b""), ("b64_clean_4", b"QUJD"), ("b64_clean_8", b"QUJDREVG"),
        ("b64_only_white_space", b" \r\n\t\x0c \r\n"),
        ("b64_one_pad", b"QUI="), ("b64_two_pads", b"QQ=="),
        ("b64_vt_inside", b"QUJD\x0bREVG"),
        ("b64_pad_in_the_middle", b"QUI=REVG"), ("b64_pad_in_the_middle_of_a_quad", b"QU=DREVG"), ("b64_three_pads", b"Q==="),
        ("b64_missing_padding", b"QUJDRA"), ("b64_missing_one_pad", b"QUJDREU"), ("b64_one_character", b"Q"), ("b64_lone_pad", b"="),
        ("b64_five_left", b"QUJDR"), ("b64_trailing_bits_two_pads", b"QR=="), ("b64_trailing_bits_one_pad", b"QUJ="),
        ("b64_char_beats_length", b"QUJ!R"), ("b64_outside_alphabet", b"QUJD-EVG"), ("b64_lines", base64.encodebytes(bytes(range(200))).replace(b"\n", b"\r\n")),
        ("b64_three_steps_and_a_byte", enc(3 * W * 3 // 4 + 30)[:3 * W] + b"\n"),
    ]
    # a quad across every step edge: white space in front so that the quad's characters lie at W-1 | W and at W-3 .. W+1
    for lead in range(W - 4, W + 2):
        out.append((f"b64_quad_from_{lead}", b" " * lead + b"QUJDREVGR0hJ"))
    out.append(("b64_white_space_inside_a_quad_at_the_edge", b"QUJD" * 15 + b"QU" + b"\r\n" * 2 + b"JD" + b"REVG"))
    # the decode rounds (256 cleaned characters, two at least stay behind) and the staging tile
    for n in (B64_ROUND - 4, B64_ROUND, B64_ROUND + 4, B64_ROUND + 8, 2 * B64_ROUND + 4, TILE, TILE + 4, 2 * TILE + 64):
        out.append((f"b64_clean_{n}", enc(n * 3 // 4)))
    out.append(("b64_clean_259_bad_length", enc(195)[:259]))
    out.append(("b64_bad_character_in_an_early_round", enc(600)[:300] + b"\x0b" + enc(600)[300:]))
    out.append(("b64_trailing_bits_after_two_rounds", enc(600)[:-4] + b"QR=="))
    return [(n, leaf(b"base64", b)) for n, b in out]


QP_EXAMPLES = [           # the worked examples of include/zkemail_amd.h, rule 9
    (b"a=\r\nb", b"ab"), (b"a \t\r\nb\r\n", b"a\r\nb"), (b"a= \r\nb", b"ab"), (b"=4", b"=4"), (b"=zz=41", b"=zzA"), (b"==41", b"==41"),
    (b"a\xffb\nc\r\r\nd", b"ab\r\nc\r\nd"), (b"\r\n\r\n", b"\r\n"),
]


def qp_cases() -> List[Tuple[str, bytes]]:
    out = [(f"qp_example_{k}", src) for k, (src, _) in enumerate(QP_EXAMPLES)]
    out += [("qp_empty", b""), ("qp_only_line_breaks", b"\r\n\r\n\r\n\r\n"), ("qp_only_lf", b"\n\n\n"), ("qp_one_lf", b"\n"),
            ("qp_soft_break_last_byte", b"abc="), ("qp_soft_break_then_white_space_at_the_end", b"abc= \t"), ("qp_cr_cr_lf", b"a\r\r\nb"),
            ("qp_lone_lf_lines", b"a\nb\n\nc\n"), ("qp_lone_cr_inside", b"a\rb\r\nc"), ("qp_trailing_white_space_at_the_end", b"abc \t \r"),
            ("qp_lower_case_hex", b"=e2=82=ac"), ("qp_mixed_case_hex", b"=eA=Ae"), ("qp_escape_then_line_end", b"=4\r\n=\r\n=41"),
            ("qp_dropped_byte_makes_an_escape", b"=\xff41 =4\x0041 =\x7f4\x801"), ("qp_control_bytes", b"a\x00b\x1fc\x7fd\x0be"),
            ("qp_high_bytes_only", b"\xff\xfe\x80"), ("qp_escape_at_the_very_end", b"abc=41"), ("qp_equals_and_one_at_the_end", b"abc=4"),
            ("qp_white_space_inside_an_escape", b"=4 1=\t41= 41"), ("qp_escape_across_a_trimmed_end", b"a=4 \r\nb=  \r\nc"),
            ("qp_lf_body_outgrows_the_email", b"\n" * 300), ("qp_lf_lines_outgrow_the_email", b"ab\n" * 400)]
    for k in range(1, 6):                                  # '=' runs: which of them start an escape
        out.append((f"qp_equals_run_{k}", b"a" + b"=" * k + b"41 b" + b"=" * k + b"\r\n" + b"=" * k))
    # an escape whose '=' lies at step offsets W-1, W-2, W-3, and at the window's edges
    for at in sorted({W - 1, W - 2, W - 3, QP_WIN - 1, QP_WIN - 2, QP_WIN, QP_WIN + 1, 2 * QP_WIN - 1, 2 * W - 1}):
        out.append((f"qp_escape_at_{at}", b"x" * at + b"=41y=4Z"))
        out.append((f"qp_soft_break_at_{at}", b"x" * at + b"=\r\nz"))
        out.append((f"qp_equals_pair_at_{at}", b"x" * at + b"==41=="))
    # white space in front of a line end that lies just behind a step (and window) edge: runs of 1, 2 and W + 1
    for run in (1, 2, W + 1):
        for edge in (W, QP_WIN, 2 * W):
            for eol_name, eol in (("crlf", b"\r\n"), ("lf", b"\n")):
                lead = max(edge - run, 1)
                out.append((f"qp_white_space_{run}_before_{eol_name}_at_{edge}", b"y" * lead + b" \t"[run % 2:run % 2 + 1] * run + eol + b"next"))
    out.append(("qp_white_space_run_then_text", b"a" + b" " * (W + 1) + b"b\r\n"))
    out.append(("qp_soft_break_before_a_long_run", b"a=" + b" " * (2 * W + 3) + b"\r\nb"))
    out.append(("qp_escape_candidate_before_a_long_run", b"a=4" + b"\t" * (2 * W) + b"\r\nb=" + b" " * (W - 2) + b"41"))
    out.append(("qp_three_tiles", (b"line =3D one=20\r\n" + b"soft=\r\nbreak \t\r\n") * 100))
    return [(n, leaf(b"quoted-printable", b)) for n, b in out]


H = b"From: a@example.com\r\nMIME-Version: 1.0\r\nContent-Type: multipart/alternative; boundary=\"xx\"\r\n\r\n"
PLAIN = b"Content-Type: text/plain\r\n\r\nplain text\r\n"
HTML = b"Content-Type: text/html\r\nContent-Transfer-Encoding: base64\r\n\r\nPGI+aGk8L2I+\r\n"
HTML_QP = b"Content-Type: text/html; charset=utf-8\r\nContent-Transfer-Encoding: quoted-printable\r\n\r\n<p>caf=C3=A9=\r\n!</p>\r\n"


def selection_cases() -> List[Tuple[str, bytes]]:
    cte = lambda v: H + b"--xx\r\nContent-Type: text/html\r\nContent-Transfer-Encoding:" + v + b"\r\n\r\nPGI+aGk8L2I+\r\n--xx--\r\n"
    return [
        ("sel_html_second_of_three", H + b"pre\r\n--xx\r\n" + PLAIN + b"--xx\r\n" + HTML + b"--xx\r\nContent-Type: image/png\r\n\r\nxyz\r\n--xx--\r\n"),
        ("sel_html_qp", H + b"--xx\r\n" + PLAIN + b"--xx\r\n" + HTML_QP + b"--xx--\r\n"),
        ("sel_two_html_first_wins", H + b"--xx\r\n" + HTML_QP + b"--xx\r\n" + HTML + b"--xx--\r\n"),
        ("sel_html_only_nested", b"From: a\r\nContent-Type: multipart/mixed; boundary=out\r\n\r\n--out\r\nContent-Type: multipart/alternative; boundary=in\r\n\r\n"
                                 b"inner preamble\r\n--in\r\n" + PLAIN + b"--in\r\n" + HTML + b"--in--\r\n--out\r\n" + PLAIN + b"--out--\r\n"),
        ("sel_nested_without_preamble", b"From: a\r\nContent-Type: multipart/mixed; boundary=out\r\n\r\n--out\r\nContent-Type: multipart/alternative; boundary=in\r\n\r\n"
                                        b"--in\r\n" + HTML + b"--in--\r\n--out--\r\n"),
        ("sel_no_children_leaf", b"From: a\r\nContent-Type: text/html\r\nContent-Transfer-Encoding: base64\r\n\r\nPGI+aGk8L2I+\r\n"),
        ("sel_no_content_type", b"From: a\r\n\r\njust text\r\n"),
        ("sel_no_headers_at_all", b"\r\nbody only"),
        ("sel_no_body", b"From: a\r\nContent-Type: multipart/mixed; boundary=xx\r\n\r\n"),
        ("sel_no_empty_line", b"From: a\r\nSubject: s\r\n"),
        ("sel_boundary_never_found", H + b"no boundary line here\r\n-- xx\r\n"),
        ("sel_first_boundary_only", H + b"preamble\r\n--xx\r\n" + HTML),
        ("sel_last_part_without_closing_boundary", H + b"--xx\r\n" + PLAIN + b"--xx\r\n" + HTML),
        ("sel_empty_first_part", H + b"--xx\r\n--xx\r\n" + PLAIN + b"--xx--\r\n"),
        ("sel_part_without_header_end", H + b"--xx\r\nContent-Type: text/html\r\n--xx--\r\n"),
        ("sel_child_content_type_upper_with_parameter", H + b"--xx\r\n" + PLAIN + b"--xx\r\nContent-Type: TEXT/HTML; charset=x\r\n\r\n<i>x</i>\r\n--xx--\r\n"),
        ("sel_child_content_type_leading_white_space", H + b"--xx\r\n" + PLAIN + b"--xx\r\nContent-Type:\t text/html ;x=y\r\n\r\n<i>y</i>\r\n--xx--\r\n"),
        ("sel_child_content_type_folded_in_front", H + b"--xx\r\n" + PLAIN + b"--xx\r\nContent-Type:\r\n text/html\r\n\r\n<i>z</i>\r\n--xx--\r\n"),
        ("sel_child_content_type_folded_inside", H + b"--xx\r\n" + PLAIN + b"--xx\r\nContent-Type: text/\r\n html\r\n\r\n<i>z</i>\r\n--xx--\r\n"),
        ("sel_child_content_type_almost_html", H + b"--xx\r\nContent-Type: text/htmlx\r\n\r\nno\r\n--xx\r\nContent-Type: text/htm\r\n\r\nno\r\n--xx--\r\n"),
        ("sel_second_content_type_is_html", H + b"--xx\r\nContent-Type: text/plain\r\nContent-Type: text/html\r\n\r\nfirst wins\r\n--xx--\r\n"),
        ("sel_lf_line_ends", H.replace(b"\r\n", b"\n") + b"--xx\n" + HTML.replace(b"\r\n", b"\n") + b"--xx--\n"),
        ("sel_body_ends_without_line_break", H + b"--xx\r\nContent-Type: text/html\r\n\r\n--xx--\r\n"),
        ("sel_body_is_one_line_break", H + b"--xx\r\nContent-Type: text/html\r\n\r\n\r\n--xx--\r\n"),
        ("sel_body_is_one_lf", H + b"--xx\r\nContent-Type: text/html\r\n\r\n\n--xx--\r\n"),
        ("sel_cr_without_lf_before_the_boundary", H + b"--xx\r\nContent-Type: text/html\r\n\r\nabc\r\r\n--xx--\r\n"),
        ("cte_upper_case", cte(b" BASE64")), ("cte_mixed_case_qp", cte(b" Quoted-Printable")), ("cte_tab_in_front", cte(b"\tbase64")),
        ("cte_folded", cte(b"\r\n base64")), ("cte_folded_inside", cte(b" base\r\n 64")), ("cte_trailing_space", cte(b" base64 ")),
        ("cte_with_comment", cte(b" base64 (x)")), ("cte_7bit", cte(b" 7bit")), ("cte_empty", cte(b"")),
        ("cte_encoded_word", cte(b" =?utf-8?q?base64?=")), ("cte_not_even_a_word", cte(b" base64=?")), ("cte_high_byte", cte(b" base64\xa0")),
        ("cte_second_header_ignored", H + b"--xx\r\nContent-Type: text/html\r\nContent-Transfer-Encoding: 7bit\r\nContent-Transfer-Encoding: base64\r\n\r\nPGI+\r\n--xx--\r\n"),
        ("cte_of_the_message_does_not_reach_the_part", H.replace(b"\r\n\r\n", b"\r\nContent-Transfer-Encoding: base64\r\n\r\n") + b"--xx\r\n" + PLAIN + b"--xx--\r\n"),
        ("cte_base64_broken_in_the_html_part", H + b"--xx\r\nContent-Type: text/html\r\nContent-Transfer-Encoding: base64\r\n\r\nPGI+aGk8L2I\r\n--xx--\r\n"),
        ("u_content_type_of_a_later_child", H + b"--xx\r\n" + HTML + b"--xx\r\nContent-Type: text/pl\xc3\xa4in\r\n\r\nx\r\n--xx--\r\n"),
        ("u_content_type_encoded_word_first_child", H + b"--xx\r\nContent-Type: =?utf-8?q?text/html?=\r\n\r\nx\r\n--xx--\r\n"),
        ("fail_child_leading_space", H + b"--xx\r\n" + HTML + b"--xx\r\n bad\r\n--xx--\r\n"),
        ("fail_top_lone_cr", b"From: a\r\n\rX: y\r\n\r\nbody"),
        ("empty_input", b""),
    ]


def all_cases() -> List[Tuple[str, bytes]]:
    return b64_cases() + qp_cases() + selection_cases()


# ------------------------------------------------------------------ the seeded generator
_WORDS = [b"<p>", b"</p>", b"<a href=3D\"x\">", b"caf\xc3\xa9 ", b"hello ", b"world", b"=", b" ", b"\t", b"1234567890", b"<br/>", b"zk-email ", b"\xe2\x82\xac"]


def _payload(rng: random.Random) -> bytes:
    n = rng.choice([0, 1, 3, 20, 60, 200, 700, 1500, 3000])
    out = bytearray()
    while len(out) < n:
        out += rng.choice(_WORDS)
        if rng.random() < 0.08:
            out += b"\r\n"
    return bytes(out[:n])


def _encode(rng: random.Random, kind: int, data: bytes, eol: bytes) -> bytes:
    """`data` under the transfer encoding `kind`, mostly as a mail client writes it, now and then broken."""
    r = rng.random()
    if kind == 1:
        text = base64.encodebytes(data).replace(b"\n", eol)
        if r < 0.06 and len(text) > 8:
            pos = rng.randrange(len(text) - 4)
            text = text[:pos] + rng.choice([b"\x0b", b"=", b"!", b""]) + text[pos + 1:]
        elif r < 0.10:
            text = text.rstrip(b"\r\n=")
        elif r < 0.14:
            text = text.rstrip(b"\r\n") + b" \t" + eol + eol
        return text
    if kind == 2:
        text = quopri.encodestring(data).replace(b"\n", eol)
        if r < 0.08:
            text += rng.choice([b"=", b"=4", b" \t", b"=zz", b"==41", b"\xff=41"])
        elif r < 0.14 and text:
            pos = rng.randrange(len(text))
            text = text[:pos] + rng.choice([b" \t ", b"\x00", b"\r", b"=", b"\n"]) + text[pos:]
        return text
    return data


_CTE_NAMES = {0: [None, b"7bit", b"8bit", b"binary", b"base64 ", b"x-uuencode"], 1: [b"base64", b"BASE64", b"Base64", b"\tbase64"],
              2: [b"quoted-printable", b"Quoted-Printable", b"QUOTED-PRINTABLE"]}


def _leaf_part(rng: random.Random, eol: bytes, ctype: bytes | None) -> bytes:
    kind = rng.choice([0, 1, 1, 2, 2])
    name = rng.choice(_CTE_NAMES[kind])
    if rng.random() < 0.015:
        name = rng.choice([b"=?utf-8?q?base64?=", b"base64\xc2\xa0", b"\r\n base64"])
        kind = rng.choice([0, 1])
    lines = []
    if ctype is not None:
        lines.append(rng.choice([b"Content-Type: ", b"content-type:", b"CONTENT-TYPE:\t"]) + ctype)
    if name is not None:
        lines.append(rng.choice([b"Content-Transfer-Encoding: ", b"content-transfer-encoding:"]) + name)
    if rng.random() < 0.3:
        lines.insert(rng.randrange(len(lines) + 1), b"Content-Disposition: inline")
    if rng.random() < 0.03:
        lines.insert(rng.randrange(len(lines) + 1), rng.choice([b" leading space", b"\rlone: cr"]))
    head = b"".join(ln + eol for ln in lines) + eol
    body = _encode(rng, kind, _payload(rng), eol)
    if body and rng.random() < 0.85 and not body.endswith(b"\n"):
        body += eol
    return head + body


_LEAF_TYPES = [b"text/plain", b"text/plain; charset=utf-8", b"text/html", b"text/html; charset=\"utf-8\"", b"TEXT/HTML", b" text/html ;x=y",
               b"image/png", b"application/octet-stream; name=\"a;b\"", None, b"text/htmlx", b""]


def generate(rng: random.Random) -> bytes:
    """One e-mail: mostly a multipart/alternative or /mixed as mail clients write them, with the defects that decide something."""
    eol = b"\r\n" if rng.random() < 0.8 else b"\n"
    top = [b"From: sender@example.com", b"To: rcpt@example.org", b"Subject: generated " + str(rng.randrange(10 ** 6)).encode(), b"MIME-Version: 1.0"]
    if rng.random() < 0.12:                               # no multipart at all
        part = _leaf_part(rng, eol, rng.choice(_LEAF_TYPES))
        return b"".join(ln + eol for ln in top) + part

    def multipart(depth: int) -> Tuple[bytes, bytes]:
        bound = rng.choice([b"b1", b"=_Part_42", b"xx", b"----=_NextPart", b"b"]) + str(depth).encode()
        ct = rng.choice([b"multipart/alternative", b"multipart/mixed", b"Multipart/Related"]) + rng.choice([b"; ", b";" + eol + b"\t"]) + \
            b"boundary=" + rng.choice([b"\"%s\"", b"%s"]) % bound
        if rng.random() < 0.01:
            ct = rng.choice([b"multipart/mixed; boundary=\"" + bound + b"\xc3\xa9\"", b"multipart/mixed; boundary*0=" + bound])
        body = b"This is a multi-part message." + eol if rng.random() < 0.4 else b""
        for _ in range(rng.choice([0, 1, 2, 2, 3, 3, 4])):
            body += b"--" + bound + eol
            if depth < 2 and rng.random() < 0.2:
                ict, ibody = multipart(depth + 1)
                body += b"Content-Type: " + ict + eol + eol + ibody
            else:
                lt = rng.choice(_LEAF_TYPES)
                if rng.random() < 0.01:
                    lt = rng.choice([b"text/html\xc2\xa0", b"=?utf-8?q?text/html?="])
                body += _leaf_part(rng, eol, lt)
        r = rng.random()
        if r < 0.85:
            body += b"--" + bound + b"--" + eol
        elif r < 0.93:
            body += b"--" + bound + eol + b"Content-Type: text/html" + eol + eol + b"never closed" + eol
        return ct, body

    ct, body = multipart(0)
    top.insert(rng.randrange(1, len(top) + 1), b"Content-Type: " + ct)
    return b"".join(ln + eol for ln in top) + eol + body


def generated(seed: int, n: int) -> List[bytes]:
    rng = random.Random(seed)
    return [generate(rng) for _ in range(n)]
