"""GPU: capture-group extraction on the device (zke_capture_batch, zke_extract_captures; csrc/capture.hip.h) against Python's
`re` (byte mode) and the `regex` module (Unicode mode): the semantics corpus of tests/capture_cases.py, look-around at the
span's edges, empty and non-participating groups, raw non-UTF-8 bytes, every limit at and one past its constant, a seeded
mutation fuzz, the round trip extract -> verify on the bench shapes, and extraction interleaved with verification on a
four-slot engine."""
import os
import random
import threading

import numpy as np
import pytest

import capture_cases as K
import synth
import zkemail_rs_amd as z
from zkemail_rs_amd import _abi as A
from zkemail_rs_amd import regex_compile as rc

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
FUZZ_SEEDS = [5, 77, 2026] + list(range(3000, 3000 + int(os.environ.get("ZKE_FUZZ_SEEDS", "0"))))


def expected_of(matches):
    """What zke_capture_batch must say about a haystack with these finditer matches: (code, count, span, group spans)."""
    if len(matches) != 1:
        return A.D_RE_MATCH_COUNT, min(len(matches), 2), (matches[0][0] if matches else (0, 0)), None
    return 0, 1, matches[0][0], matches[0][1]


def check_pattern(engine, pattern, unicode, hays, all_matches):
    """Every haystack through zke_capture_batch.  First with every group of the pattern requested (a haystack in which one took no
    part must say ZKE_D_RE_GROUP_MISSING), then per set of participating groups with exactly those, so that every span Python
    reports is compared.  Returns the number of single-match haystacks."""
    _, dfa_id, prog_id = engine.compile_pattern(pattern, unicode)
    assert engine.dfa_status(dfa_id) == 0 and engine.capture_status(prog_id) == 0, pattern
    exp = [expected_of(m) for m in all_matches]
    ng = K.group_count(pattern, unicode)
    groups = list(range(0, ng + 1))
    matches, spans, flags, strings = engine.capture_batch(dfa_id, prog_id, groups, hays)
    by_sig = {}
    singles = 0
    for i, (code, count, span, gs) in enumerate(exp):
        got = tuple(int(x) for x in matches[i])
        where = (pattern, hays[i], i)
        if code:
            assert got[:2] == (code, count), where
            if count:
                assert got[2:] == span, where
            assert strings[i] == [] and (spans[i] == NONE).all(), where
            continue
        singles += 1
        assert got[1:] == (1,) + span, where
        full = all(g is not None for g in gs)
        assert got[0] == (0 if full else A.D_RE_GROUP_MISSING), where
        by_sig.setdefault(tuple(k + 1 for k, g in enumerate(gs) if g is not None), []).append(i)
        if full:
            want = [span] + list(gs)
            assert [tuple(int(x) for x in s) for s in spans[i]] == want, where
            assert strings[i] == [hays[i][a:b] for a, b in want], where
    for sig, idx in by_sig.items():
        if len(sig) == ng:
            continue                                   # compared above
        sub = [hays[i] for i in idx]
        m2, s2, f2, str2 = engine.capture_batch(dfa_id, prog_id, list(sig), sub)
        for k, i in enumerate(idx):
            gs = exp[i][3]
            want = [gs[g - 1] for g in sig]
            assert int(m2[k][0]) == 0 and [tuple(int(x) for x in s) for s in s2[k]] == want, (pattern, sub[k], sig)
            assert str2[k] == [sub[k][a:b] for a, b in want]
    return singles


def test_semantics_corpus_byte_mode(engine):
    hays = K.byte_haystacks(400, 7)
    for pat in K.BYTE_PATTERNS:
        singles = check_pattern(engine, pat, False, hays, [K.byte_matches(pat, h) for h in hays])
        assert singles >= 1, pat


def test_semantics_corpus_unicode_mode(engine):
    """Unicode \\w \\d . over multi-byte text (programs of up to 6 870 states: their rows live in the slot workspace, not in LDS).
    Every haystack is valid UTF-8, so nothing is skipped."""
    texts = K.unicode_haystacks(200, 11)
    hays = [t.encode("utf-8") for t in texts]
    for pat in K.UNICODE_PATTERNS:
        singles = check_pattern(engine, pat, True, hays, [K.unicode_matches(pat, t) for t in texts])
        assert singles >= 1, pat


def one(engine, pattern, hay, groups, unicode=False):
    _, dfa_id, prog_id = engine.compile_pattern(pattern, unicode)
    m, spans, flags, strings = engine.capture_batch(dfa_id, prog_id, groups, [hay])
    return [int(x) for x in m[0]], [tuple(int(x) for x in s) for s in spans[0]], [int(f) for f in flags[0]], strings[0]


def test_look_around_sees_the_bytes_outside_the_span(engine):
    # \b on the byte just in front of / behind the match: "xab" has no boundary in front of "ab", " ab" has
    assert one(engine, r"(?-u:\b)(ab)(?-u:\b)", b"xab ab.", [1])[:2] == ([0, 1, 4, 6], [(4, 6)])
    assert one(engine, r"(?-u:\b)(ab)(?-u:\b)", b"xabx", [1])[0][:2] == [A.D_RE_MATCH_COUNT, 0]
    # (?m)^ / $ decided by the line feeds just outside the span; \A / \z by the haystack's ends, not the span's
    assert one(engine, r"(?m)^(id): (\S+)$", b"xid: 1\nid: 22\nz", [1, 2])[:2] == ([0, 1, 7, 13], [(7, 9), (11, 13)])
    assert one(engine, r"(b+)\z", b"abb abb", [1])[:2] == ([0, 1, 5, 7], [(5, 7)])
    assert one(engine, r"\A(a)|(b)\z", b"ab", [0])[0][:2] == [A.D_RE_MATCH_COUNT, 2]


def test_empty_missing_and_raw_groups(engine):
    # an empty capture is a string of length 0, not a missing group
    m, spans, flags, strings = one(engine, r"k=([0-9]*);", b"..k=;..", [1])
    assert m == [0, 1, 2, 5] and spans == [(4, 4)] and strings == [b""]
    # a group that took no part, and a group index the pattern does not have: "Capture group not found"
    assert one(engine, r"(a)|(b)", b"b", [2])[:2] == ([0, 1, 0, 1], [(0, 1)])
    assert one(engine, r"(a)|(b)", b"b", [1])[0] == [A.D_RE_GROUP_MISSING, 1, 0, 1]
    assert one(engine, r"(a)|(b)", b"b", [3])[0] == [A.D_RE_GROUP_MISSING, 1, 0, 1]
    # raw bytes come back raw; the flag says that they are not UTF-8 (byte mode: `.` takes any byte but \n)
    m, spans, flags, strings = one(engine, r"<(.*)>(x)", b"<a\xff\xfeb>x", [1, 2])
    assert m[0] == 0 and strings == [b"a\xff\xfeb", b"x"] and flags == [A.CAPF_NOT_UTF8, 0]


def test_span_limit_at_and_past(engine):
    pat = r"<([a-z]*)>"
    at = b"<" + b"a" * (A.CAP_MAX_SPAN - 2) + b">"
    m, spans, _, strings = one(engine, pat, b"--" + at + b"--", [0, 1])
    assert m == [0, 1, 2, 2 + A.CAP_MAX_SPAN] and spans == [(2, 2 + A.CAP_MAX_SPAN), (3, 1 + A.CAP_MAX_SPAN)]
    assert strings == [at, at[1:-1]]
    m, spans, _, strings = one(engine, pat, b"--<" + b"a" * (A.CAP_MAX_SPAN - 1) + b">--", [1])
    assert m == [A.D_U_CAPTURE_SPAN, 1, 2, 3 + A.CAP_MAX_SPAN] and strings == [] and spans == [(NONE, NONE)]


def pattern_with_states(n_states):
    """a(b+|c{k})d with exactly n_states program states (one state per repeated literal plus a fixed frame)."""
    base = A.CAP_MAX_STATES // 2
    have = rc.create_capture_program("a(b+|c{%d})d" % base, unicode=False)
    k = base + (n_states - int.from_bytes(have[8:12], "little"))
    pat = "a(b+|c{%d})d" % k
    assert int.from_bytes(rc.create_capture_program(pat, unicode=False)[8:12], "little") == n_states
    return pat


def test_state_limit_at_and_past(engine):
    # the span is found by the DFA pair of a(b+)d, the same language on texts without a "c" (the DFA of c{8000} is not the point)
    _, dfa_id, _ = engine.compile_pattern(r"a(b+)d", False)
    hay = b"..abbbd.."
    pid = engine.capture_register(rc.create_capture_program(pattern_with_states(A.CAP_MAX_STATES), unicode=False))
    assert engine.capture_status(pid) == 0
    matches, spans, _, strings = engine.capture_batch(dfa_id, pid, [0, 1], [hay])
    assert [int(x) for x in matches[0]] == [0, 1, 2, 7] and strings == [[b"abbbd", b"bbb"]]
    pid2 = engine.capture_register(rc.create_capture_program(pattern_with_states(A.CAP_MAX_STATES + 1), unicode=False))
    assert engine.capture_status(pid2) == A.D_U_CAPTURE_STATES
    matches, _, _, strings = engine.capture_batch(dfa_id, pid2, [1], [hay])
    assert [int(x) for x in matches[0]] == [A.D_U_CAPTURE_STATES, 1, 2, 7] and strings == [[]]
    engine.capture_unregister(pid)
    engine.capture_unregister(pid2)


def test_walk_disagrees_loudly(engine):
    """A program that is not the DFA pair's pattern cannot reproduce its span: reported, not guessed."""
    _, dfa_id, _ = engine.compile_pattern(r"a(b+)d", False)
    _, _, other = engine.compile_pattern(r"a(b{2})d", False)
    matches, spans, _, strings = engine.capture_batch(dfa_id, other, [1], [b"..abbbd..", b"abbd"])
    assert [int(x) for x in matches[0]] == [A.D_U_CAPTURE_WALK, 1, 2, 7] and [int(x) for x in matches[1]] == [0, 1, 0, 4]
    assert strings == [[], [b"bb"]]


def test_group_limits_at_and_past(engine):
    pat31 = "".join("(%s)" % chr(97 + k % 26) for k in range(A.CAP_MAX_PROGRAM_GROUPS - 1))       # 31 groups + group 0 = 32
    hay = "".join(chr(97 + k % 26) for k in range(A.CAP_MAX_PROGRAM_GROUPS - 1)).encode()
    _, dfa_id, pid = engine.compile_pattern(pat31, False)
    assert engine.capture_status(pid) == 0
    want = list(range(16, 16 + A.CAP_MAX_GROUPS))                                                  # 16 requested groups: the limit
    matches, spans, _, strings = engine.capture_batch(dfa_id, pid, want, [hay])
    assert int(matches[0][0]) == 0 and [tuple(int(x) for x in s) for s in spans[0]] == [(g - 1, g) for g in want]
    with pytest.raises(z.EngineError):                                                              # 17: refused, nothing truncated
        engine.capture_batch(dfa_id, pid, list(range(1, A.CAP_MAX_GROUPS + 2)), [hay])
    _, dfa2, pid2 = engine.compile_pattern(pat31 + "(z)", False)                                    # 33 groups in the program
    assert engine.capture_status(pid2) == A.D_U_CAPTURE_STATES
    matches, _, _, strings = engine.capture_batch(dfa2, pid2, [1], [hay + b"z"])
    assert [int(x) for x in matches[0]][:2] == [A.D_U_CAPTURE_STATES, 1] and strings == [[]]


def test_undecodable_program_and_dfa_are_reported(engine):
    _, dfa_id, pid = engine.compile_pattern(r"(a)b", False)
    bad = engine.capture_register(b"not a program")
    assert engine.capture_status(bad) == A.D_U_CAPTURE_PROGRAM
    matches, _, _, strings = engine.capture_batch(dfa_id, bad, [1], [b"ab"])
    assert [int(x) for x in matches[0]] == [A.D_U_CAPTURE_PROGRAM, 1, 0, 2] and strings == [[]]
    matches, _, _, _ = engine.capture_batch(dfa_id, 1 << 20, [1], [b"ab"])                          # an id nobody registered
    assert int(matches[0][0]) == A.D_U_CAPTURE_PROGRAM
    bad_dfa = engine.dfa_register(b"x" * 40, b"y" * 40)
    matches, _, _, _ = engine.capture_batch(bad_dfa, pid, [1], [b"ab"])
    assert int(matches[0][0]) == A.D_DFA_LABEL


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_mutation_fuzz(engine, seed):
    """Random byte edits of matching haystacks around the match: substitutions, insertions and deletions within a few bytes of
    the span's edges and inside it."""
    rng = random.Random(seed)
    alph = b"abcxyz019;=<>@. \r\n:kfeo-,ZKE"
    for pat in K.BYTE_PATTERNS:
        base = [h for h in K.byte_haystacks(300, seed) if len(K.byte_matches(pat, h)) == 1][:40]
        hays = []
        for h in base:
            (s, e), _ = K.byte_matches(pat, h)[0]
            for _ in range(6):
                m = bytearray(h)
                for _ in range(rng.randint(1, 3)):
                    at = min(max(rng.randint(s - 3, e + 3), 0), len(m))
                    op = rng.random()
                    if op < 0.5 and at < len(m):
                        m[at] = rng.choice(alph)
                    elif op < 0.75:
                        m.insert(at, rng.choice(alph))
                    elif at < len(m):
                        del m[at]
                hays.append(bytes(m))
        if hays:
            check_pattern(engine, pat, False, hays, [K.byte_matches(pat, h) for h in hays])


# ---- the e-mail entry: raw e-mails + keys + patterns in, RegexInfo tables out
def config_of(n_header_parts, n_body_parts):
    return rc.RegexConfig([rc.RegexPattern(p, ci) for p, ci in synth.HEADER_PATTERNS[:n_header_parts]] or None,
                          [rc.RegexPattern(p, ci) for p, ci in synth.BODY_PATTERNS[:n_body_parts]] or None)


def round_trip(engine, inputs, expect, cfg):
    emails = [i.email for i in inputs]
    records, infos = engine.extract_captures(emails, cfg, unicode=False)
    n_hdr = len(cfg.header_parts or [])
    for i, (inp, info, why) in enumerate(zip(inputs, infos, expect)):
        r = records[i]
        if why is None:
            assert r["status"] == A.ZKE_OK and info is not None, i
            for side in ("header_parts", "body_parts"):
                mine, theirs = getattr(info, side), getattr(inp.regex_info, side)
                assert (mine is None) == (theirs is None)
                for a, b in zip(mine or [], theirs or []):
                    assert a.captures == b.captures, (i, side)           # the strings synth derived with `re`
                    assert a.verify_re == b.verify_re
        else:                                                             # "Input doesn't match regex pattern"
            assert info is None
            assert r["status"] == (A.ZKE_HEADER_REGEX_FAIL if why == "header" else A.ZKE_BODY_REGEX_FAIL) and r["detail"] == A.D_RE_MATCH_COUNT, i
            assert r["match_count"] == 2 and r["regex_part"] == (1 if why == "header" else n_hdr), i
    # what was extracted verifies, record for record as synth's own inputs do (a failing e-mail carries no strings: its match
    # count fails before any containment test)
    empty = A.RegexInfo([A.CompiledRegex(p.verify_re, []) for p in inputs[0].regex_info.header_parts or []] or None,
                        [A.CompiledRegex(p.verify_re, []) for p in inputs[0].regex_info.body_parts or []] or None)
    mine = [A.EmailWithRegex(e, info if info is not None else empty) for e, info in zip(emails, infos)]
    got = engine.verify_emails_with_regex(mine)
    ref = engine.verify_emails_with_regex(inputs)
    for f in A.RESULT_DTYPE.names:
        assert (np.asarray(got[f]) == np.asarray(ref[f])).all(), f
    return records


def test_round_trip_c3_shape(engine):
    inputs, wl, expect = synth.make_regex_workload("c3", 512, 4096, rsa_bits=2048, n_keys=4, seed=21, n_header_parts=2, fail_frac=0.1)
    assert any(expect) and not all(expect)
    records = round_trip(engine, inputs, expect, config_of(2, 0))
    ok = [i for i, w in enumerate(expect) if w is None]
    # and the module-level spelling of the reference's function returns values verify accepts
    some = [inputs[i].email for i in ok[:8]]
    made = z.generate_email_with_regex_inputs(some, config_of(2, 0), unicode=False, engine=engine)
    assert (engine.verify_emails_with_regex(made)["status"] == A.ZKE_OK).all()
    bad = next(i for i, w in enumerate(expect) if w)
    with pytest.raises(z.VerifyPanic):
        z.generate_email_with_regex_inputs([inputs[bad].email], config_of(2, 0), unicode=False, engine=engine)
    assert len(records) == 512


def test_round_trip_c5re_shape(engine):
    inputs, wl, expect = synth.make_regex_workload("c5re", 192, 4096, rsa_bits=4096, n_keys=2, seed=22, n_header_parts=2, n_body_parts=2,
                                                   qp_frac=0.05, fail_frac=0.15)
    assert "header" in expect and "body" in expect
    round_trip(engine, inputs, expect, config_of(2, 2))


def test_dkim_failure_and_missing_group_statuses(engine):
    inputs, wl, expect = synth.make_regex_workload("c3", 16, 1024, rsa_bits=2048, n_keys=2, seed=23, n_header_parts=2)
    emails = [i.email for i in inputs]
    raw = bytearray(emails[3].raw_email)
    raw[-3] ^= 1                                                          # body hash mismatch
    emails[3] = A.Email(emails[3].from_domain, bytes(raw), emails[3].public_key)
    cfg = config_of(2, 0)
    records, infos = engine.extract_captures(emails, cfg, unicode=False)
    assert records[3]["status"] == A.ZKE_DKIM_NOT_PASS and infos[3] is None
    assert all(r["status"] == A.ZKE_OK for k, r in enumerate(records) if k != 3)
    # group 2 does not exist in the subject pattern: every e-mail is "Capture group not found", named at part 1
    cfg2 = rc.RegexConfig([rc.RegexPattern(synth.HEADER_PATTERNS[0][0], [1]), rc.RegexPattern(synth.HEADER_PATTERNS[1][0], [1, 2])], None)
    records, infos = engine.extract_captures(emails, cfg2, unicode=False)
    for k, r in enumerate(records):
        if k == 3:
            assert r["status"] == A.ZKE_DKIM_NOT_PASS
        else:
            assert (r["status"], r["detail"], r["regex_part"], r["match_count"]) == (A.ZKE_HEADER_REGEX_FAIL, A.D_RE_GROUP_MISSING, 1, 1)
        assert infos[k] is None


def test_one_fold_over_match_counts_and_captures(engine):
    """compile_regex_parts walks part by part — a part's match count, then its groups, then the next part — so the record names
    the FIRST part that fails for either reason: a missing group in part 0 comes in front of two matches in part 1, and two matches
    in part 0 in front of a missing group in part 1."""
    inputs, wl, expect = synth.make_regex_workload("c3", 64, 1024, rsa_bits=2048, n_keys=2, seed=25, n_header_parts=2, fail_frac=0.4)
    assert "header" in expect and None in expect            # 'header': two Subject headers signed, the subject pattern matches twice
    emails = [i.email for i in inputs]
    frm, subj = synth.HEADER_PATTERNS[0][0], synth.HEADER_PATTERNS[1][0]
    # part 0: the from pattern with a group it does not have; part 1: the subject pattern
    records, infos = engine.extract_captures(emails, rc.RegexConfig([rc.RegexPattern(frm, [1, 2]), rc.RegexPattern(subj, [1])], None), unicode=False)
    for r, info in zip(records, infos):
        assert (r["status"], r["detail"], r["regex_part"], r["match_count"]) == (A.ZKE_HEADER_REGEX_FAIL, A.D_RE_GROUP_MISSING, 0, 1) and info is None
    # the reverse: part 0 the subject pattern, part 1 the from pattern with the missing group
    records, infos = engine.extract_captures(emails, rc.RegexConfig([rc.RegexPattern(subj, [1]), rc.RegexPattern(frm, [1, 2])], None), unicode=False)
    for r, info, why in zip(records, infos, expect):
        want = (A.ZKE_HEADER_REGEX_FAIL, A.D_RE_MATCH_COUNT, 0, 2) if why else (A.ZKE_HEADER_REGEX_FAIL, A.D_RE_GROUP_MISSING, 1, 1)
        assert (r["status"], r["detail"], r["regex_part"], r["match_count"]) == want and info is None
    # an unusable program (beyond the state limit) in part 0 in front of two matches in part 1: ZKE_UNSUPPORTED names part 0.
    # (a(b+|c{k})d never matches a header, so its own DFA pair would report a match count of 0 first: the from pattern's pair
    # finds the span, the oversized program is what would have to walk it)
    big = engine.capture_register(rc.create_capture_program(pattern_with_states(A.CAP_MAX_STATES + 1), unicode=False))
    _, frm_dfa, _ = engine.compile_pattern(frm, False)
    _, subj_dfa, subj_prog = engine.compile_pattern(subj, False)
    records = raw_extract(engine, emails, [(frm_dfa, big, [1]), (subj_dfa, subj_prog, [1])], 2, 0)
    for r in records:
        assert (r["status"], r["detail"], r["regex_part"], r["match_count"]) == (A.ZKE_UNSUPPORTED, A.D_U_CAPTURE_STATES, 0, 1)
    records = raw_extract(engine, emails, [(subj_dfa, subj_prog, [1]), (frm_dfa, big, [1])], 2, 0)
    for r, why in zip(records, expect):
        want = (A.ZKE_HEADER_REGEX_FAIL, A.D_RE_MATCH_COUNT, 0, 2) if why else (A.ZKE_UNSUPPORTED, A.D_U_CAPTURE_STATES, 1, 1)
        assert (r["status"], r["detail"], r["regex_part"], r["match_count"]) == want
    engine.capture_unregister(big)


def raw_extract(engine, emails, parts, n_header, n_body, expect_rc=0):
    """zke_extract_captures with explicit (dfa id, program id, groups) per part."""
    import ctypes as C
    arr = (A.zke_capture_part * len(parts))()
    keep = []
    for k, (d, p, g) in enumerate(parts):
        ga = np.array(g, np.uint32)
        keep.append(ga)
        arr[k].dfa_id, arr[k].prog_id, arr[k].n_groups, arr[k].groups = d, p, len(g), ga.ctypes.data
    refs = A.EmailRefs(emails)
    n, P, G = refs.n, len(parts), sum(len(g) for _, _, g in parts)
    out = np.zeros(max(n, 1), dtype=A.RESULT_DTYPE)
    body = C.cast(C.byref(arr, n_header * C.sizeof(A.zke_capture_part)), C.POINTER(A.zke_capture_part))
    rcode, *_ = engine._run_captures(n, P, G, lambda o: engine.lib.zke_extract_captures(engine.h, refs.arr, n, arr, n_header, body, n_body,
                                                                                      out.ctypes.data, C.byref(o)), 64 * n * G)
    assert rcode == expect_rc, rcode
    return out[:n]


def test_part_limit_at_and_past(engine):
    inputs, wl, expect = synth.make_regex_workload("c3", 4, 1024, rsa_bits=2048, n_keys=1, seed=26, n_header_parts=2)
    emails = [i.email for i in inputs]
    frm = synth.HEADER_PATTERNS[0][0]
    want = inputs[0].regex_info.header_parts[0].captures
    records, infos = engine.extract_captures(emails[:1], rc.RegexConfig([rc.RegexPattern(frm, [1])] * A.CAP_MAX_PARTS, None), unicode=False)
    assert records[0]["status"] == A.ZKE_OK and [p.captures for p in infos[0].header_parts] == [want] * A.CAP_MAX_PARTS
    # half of them as body parts: the limit is on the sum (the from pattern does not match a body: part 8, match count 0)
    records, infos = engine.extract_captures(emails, rc.RegexConfig([rc.RegexPattern(frm, [1])] * 8, [rc.RegexPattern(frm, [1])] * 8), unicode=False)
    assert all((r["status"], r["detail"], r["regex_part"], r["match_count"]) == (A.ZKE_BODY_REGEX_FAIL, A.D_RE_MATCH_COUNT, 8, 0) for r in records)
    with pytest.raises(z.EngineError):                       # 17: refused as a call, nothing is dropped silently
        engine.extract_captures(emails, rc.RegexConfig([rc.RegexPattern(frm, [1])] * (A.CAP_MAX_PARTS + 1), None), unicode=False)
    with pytest.raises(z.EngineError):
        engine.extract_captures(emails, rc.RegexConfig([rc.RegexPattern(frm, [1])] * 9, [rc.RegexPattern(frm, [1])] * 8), unicode=False)


def test_extraction_interleaved_with_verification_on_four_slots():
    """Extraction batches and verify batches from two host threads on a 4-slot engine give what a serial run gives."""
    eng = z.Engine(slots=4)
    try:
        inputs, wl, expect = synth.make_regex_workload("c3", 96, 1024, rsa_bits=2048, n_keys=2, seed=24, n_header_parts=2, fail_frac=0.1)
        emails = [i.email for i in inputs]
        cfg = config_of(2, 0)
        chunks = [slice(k, k + 24) for k in range(0, 96, 24)]
        serial_x = [eng.extract_captures(emails[c], cfg, unicode=False) for c in chunks]
        serial_v = [eng.verify_emails_with_regex(inputs[c]) for c in chunks]
        got = {}

        def extractor():
            for rep in range(3):
                for k, c in enumerate(chunks):
                    got[("x", rep, k)] = eng.extract_captures(emails[c], cfg, unicode=False)

        def verifier():
            for rep in range(3):
                for k, c in enumerate(chunks):
                    got[("v", rep, k)] = eng.verify_emails_with_regex(inputs[c])

        ts = [threading.Thread(target=extractor), threading.Thread(target=verifier)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        for rep in range(3):
            for k in range(len(chunks)):
                rx, ix = got[("x", rep, k)]
                assert rx.tobytes() == serial_x[k][0].tobytes() and ix == serial_x[k][1]
                assert got[("v", rep, k)].tobytes() == serial_v[k].tobytes()
    finally:
        eng.close()
