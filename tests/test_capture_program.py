"""CPU (-m "not gpu"): the capture program (zkemail_rs_amd.regex_compile.create_capture_program) and its host reader.

  * tests/capture_model.py interprets the BLOB — decode, leftmost-first Pike simulation — and must agree with Python's `re`
    (byte mode) and with the `regex` module (Unicode mode; character offsets converted to bytes) on the overall span and on
    every group span of every finditer match of the corpus in tests/capture_cases.py;
  * three golden blobs pin the format;
  * every truncation and 10 000 random word substitutions of the golden blobs are either refused by the engine's host reader
    (zke_capture_validate, no GPU involved) or walk inside their tables;
  * the new entry points refuse null arguments; the ctypes mirrors have the header's layout."""
import ctypes as C
import os
import random
import struct

import numpy as np
import pytest

import capture_cases as K
import capture_model as M
from zkemail_rs_amd import _abi as A
from zkemail_rs_amd import engine
from zkemail_rs_amd import regex_compile as rc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_PROGRAMS = [("capture_from_header.zkcp", r"from:[^\r\n]*<([a-z]+)@example\.com>\r\n", False),
                   ("capture_alternation.zkcp", r"(a|ab)(c|bcd)(d*)", False),
                   ("capture_unicode_lazy.zkcp", r"<(.+?)>", True)]


def flat(span, groups):
    out = [span[0], span[1]]
    for g in groups:
        out += [None, None] if g is None else list(g)
    return out


def test_model_agrees_with_re_in_byte_mode():
    hays = K.byte_haystacks(400, 7)
    total = 0
    for pat in K.BYTE_PATTERNS:
        prog = M.Program(rc.create_capture_program(pat, unicode=False))
        assert not prog.unicode and prog.n_groups == K.group_count(pat, False) + 1
        for h in hays:
            for span, groups in K.byte_matches(pat, h):
                assert M.captures_at(prog, h, span[0]) == flat(span, groups), (pat, h, span)
                total += 1
    assert total > 3000


def test_model_agrees_with_regex_in_unicode_mode():
    texts = K.unicode_haystacks(200, 11)
    total = 0
    for pat in K.UNICODE_PATTERNS:
        prog = M.Program(rc.create_capture_program(pat, unicode=True))
        assert prog.unicode
        for t in texts:
            h = t.encode("utf-8")
            for span, groups in K.unicode_matches(pat, t):
                assert M.captures_at(prog, h, span[0]) == flat(span, groups), (pat, t, span)
                total += 1
    assert total > 500


def test_group_numbers_do_not_change_the_dfa_pair():
    """The parser now keeps group indices; create_dfa must not see them: a pattern and its non-capturing spelling give one DFA pair."""
    for a, b in ((r"x(ab|a)(bc|c)?y?", r"x(?:ab|a)(?:bc|c)?y?"), (r"(?:k(\d)+,)+z", r"(?:k(?:\d)+,)+z")):
        assert rc.create_dfa(a) == rc.create_dfa(b)


def test_the_unicode_from_pattern_fits_the_state_limit():
    blob = rc.create_capture_program(r"from:[^\r\n]*<(\w+)@([\w.]+)>", unicode=True)
    n_states = struct.unpack_from("<I", blob, 8)[0]
    assert n_states <= A.CAP_MAX_STATES == M.MAX_STATES == rc.CAP_MAX_STATES
    assert validate(blob) == 0
    assert A.CAP_MAX_GROUPS >= 16 and A.CAP_MAX_SPAN >= 4096 and A.CAP_MAX_PROGRAM_GROUPS == M.MAX_PROGRAM_GROUPS


def test_golden_blobs_pin_the_format():
    for name, pat, uni in GOLDEN_PROGRAMS:
        blob = open(os.path.join(GOLDEN, name), "rb").read()
        assert rc.create_capture_program(pat, unicode=uni) == blob, f"{name}: the compiler's output changed; the format is versioned"
        magic, version, n_states, n_groups, start, flags, n_words, zero = struct.unpack_from("<8I", blob)
        assert (magic, version, flags, zero) == (rc.CAP_MAGIC, 1, int(uni), 0) and blob[:4] == b"ZKCP"
        assert len(blob) == 4 * (8 + n_states + 1 + n_words) and start < n_states
        assert validate(blob) == 0


def validate(blob: bytes) -> int:
    lib = engine.load_library()
    d = C.c_uint32(0xFFFF)
    buf = np.frombuffer(bytes(blob) or b"\0", np.uint8)
    assert lib.zke_capture_validate(buf.ctypes.data, len(blob), C.byref(d)) == 0
    return d.value


def model_verdict(blob: bytes) -> int:
    try:
        M.Program(blob)
        return 0
    except M.BadProgram as e:
        return e.detail


def test_host_reader_refuses_or_stays_inside_the_tables():
    """The engine's host reader and the model's decoder state the same rules, so they must give the same verdict on every
    mutation; and a mutation both accept is then WALKED by the model, whose list indexing raises on any index outside a table."""
    rng = random.Random(20260)
    hays = K.byte_haystacks(12, 3) + [t.encode() for t in K.unicode_haystacks(6, 3)]
    accepted = 0
    for name, _, _ in GOLDEN_PROGRAMS:
        blob = open(os.path.join(GOLDEN, name), "rb").read()
        for cut in range(len(blob)):                                  # every truncation
            got = validate(blob[:cut])
            assert got == model_verdict(blob[:cut]) != 0, (name, cut)
        words = list(struct.unpack(f"<{len(blob) // 4}I", blob))
        n_states = words[2]
        for k in range(10000 // len(GOLDEN_PROGRAMS) + 1):            # random word substitutions
            w = list(words)
            for _ in range(rng.choice((1, 1, 2))):
                at = rng.randrange(len(w))
                w[at] = rng.choice((rng.randrange(1 << 32), rng.randrange(n_states + 2), rng.randrange(8), w[at] ^ (1 << rng.randrange(32)),
                                    rng.randrange(256) | rng.randrange(256) << 8, 0xFFFFFFFF, 0))
            mut = struct.pack(f"<{len(w)}I", *w)
            got = validate(mut)
            assert got == model_verdict(mut), (name, k)
            if got == 0:
                accepted += 1
                prog = M.Program(mut)
                for h in hays[:4] if accepted % 8 else hays:
                    for start in range(0, len(h) + 1, 3):
                        M.captures_at(prog, h, start)                 # IndexError here = the reader let an index through
    assert accepted > 500


def test_limits_are_reported_not_truncated():
    many = "".join("(%s)" % chr(97 + k % 26) for k in range(A.CAP_MAX_PROGRAM_GROUPS))           # 32 groups + group 0
    assert validate(rc.create_capture_program(many[:-3], unicode=False)) == 0
    assert validate(rc.create_capture_program(many, unicode=False)) == A.D_U_CAPTURE_STATES
    assert validate(rc.create_capture_program("a{%d}" % A.CAP_MAX_STATES, unicode=False)) == A.D_U_CAPTURE_STATES
    assert validate(b"") == validate(b"ZKCP") == A.D_U_CAPTURE_PROGRAM


def test_struct_layouts_and_constants():
    assert C.sizeof(A.zke_capture_part) == 24 and A.zke_capture_part.groups.offset == 16
    assert C.sizeof(A.zke_capture_out) == 128 and A.zke_capture_out.spans_need.offset == 80 and A.zke_capture_out.n_strings.offset == 120
    assert C.sizeof(A.zke_options) == 104 and C.sizeof(A.zke_timings) == 32 and C.sizeof(A.zke_result) == 192        # ABI 0.3: additions only
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "zkemail_amd.h")).read()
    for name, val in (("ZKE_CAP_MAX_STATES", A.CAP_MAX_STATES), ("ZKE_CAP_MAX_PROGRAM_GROUPS", A.CAP_MAX_PROGRAM_GROUPS),
                      ("ZKE_CAP_MAX_GROUPS", A.CAP_MAX_GROUPS), ("ZKE_CAP_MAX_SPAN", A.CAP_MAX_SPAN), ("ZKE_CAP_MAX_PARTS", A.CAP_MAX_PARTS),
                      ("ZKE_CAPF_NOT_UTF8", A.CAPF_NOT_UTF8)):
        assert f"#define {name} {val}u" in " ".join(hdr.split()), name
    used = {}
    import re
    for m in re.finditer(r"\b(ZKE_D_[A-Z0-9_]+)\s*=\s*(\d+)", hdr):                   # new detail codes take unused numbers
        assert int(m.group(2)) not in used, (m.group(1), used.get(int(m.group(2))))
        used[int(m.group(2))] = m.group(1)


def test_null_arguments_are_refused_not_dereferenced():
    lib = engine.load_library()
    E_ARG = -1
    u, t = C.c_uint32(), C.c_uint64()
    o = A.zke_capture_out()
    out = np.zeros(1, dtype=A.RESULT_DTYPE)
    part = A.zke_capture_part()
    assert lib.zke_capture_register(None, None, 0, C.byref(u)) == E_ARG
    assert lib.zke_capture_status(None, 0, C.byref(u)) == E_ARG and lib.zke_capture_unregister(None, 0) == E_ARG
    assert lib.zke_capture_validate(None, 4, C.byref(u)) == E_ARG and lib.zke_capture_validate(None, 0, None) == E_ARG
    assert lib.zke_extract_captures(None, None, 0, C.byref(part), 1, None, 0, out.ctypes.data, C.byref(o)) == E_ARG
    assert lib.zke_extract_captures_async(None, None, 0, C.byref(part), 1, None, 0, out.ctypes.data, C.byref(o), C.byref(t)) == E_ARG
    assert lib.zke_capture_batch(None, 0, 0, None, 0, None, None, 0, None, C.byref(o)) == E_ARG
