"""GPU: the index map of remove_quoted_printable_soft_breaks on the device (csrc/qpmap.hip.h) — zke_qp_clean_batch bit for bit against
the model of tests/qp_map_model.py, the origins zke_extract_captures_mapped reports against the model applied to the oracle's
canonical body, the mapped extraction against the plain one, and the C++ mirror through tests/cpp/qpmap_test."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import qp_map_model as Q
import synth
import zkemail_rs_amd as z
from zkemail_rs_amd import _abi as A
from zkemail_rs_amd import build
from zkemail_rs_amd import regex_compile as rc

pytestmark = pytest.mark.gpu

NO = Q.NO_INDEX


# ---- zke_qp_clean_batch
def qp_call(engine, blob, off, n, total, want=(True, True, True)):
    cleaned, imap, clen = np.full(max(total, 1), 0xAA, np.uint8), np.full(max(total, 1), 0xAAAAAAAA, np.uint32), np.full(max(n, 1), 0xAAAAAAAA, np.uint32)
    rcode = engine.lib.zke_qp_clean_batch(engine.h, blob.ctypes.data, off.ctypes.data, n, cleaned.ctypes.data if want[0] else None,
                                          imap.ctypes.data if want[1] else None, clen.ctypes.data if want[2] else None)
    assert rcode == 0, engine.lib.zke_last_error(None)
    return cleaned, imap, clen


def test_index_map_cases(engine):
    bodies = Q.cases()
    ref = [Q.remove_qp(b) for b in bodies]
    cleaned, maps, clen = engine.qp_clean_batch(bodies)
    for b, (c, im, kept), gc, gm, gl in zip(bodies, ref, cleaned, maps, clen):
        assert gc == c and gm.tolist() == im and int(gl) == kept, b[:80]
    # body_off[0] != 0 (the bytes in front belong to nobody), and each single output absent in turn
    some = bodies[:64]
    blob, off = A._csr([b"\xff" * 37] + some)
    total = int(off[-1] - off[1])
    want_c = b"".join(r[0] for r in ref[:64])
    want_m = [x for r in ref[:64] for x in r[1]]
    want_l = [r[2] for r in ref[:64]]
    for want in ((True, True, True), (False, True, True), (True, False, True), (True, True, False), (False, False, True)):
        c, m, ln = qp_call(engine, blob, off[1:].copy(), len(some), total, want)
        assert (c[:total].tobytes() == want_c) if want[0] else (c == 0xAA).all()
        assert (m[:total].tolist() == want_m) if want[1] else (m == 0xAAAAAAAA).all()
        assert (ln.tolist() == want_l) if want[2] else (ln == 0xAAAAAAAA).all()
    # n == 0 touches nothing; the reference's own pair for one body
    c, m, ln = qp_call(engine, blob, off, 0, 8)
    assert (c == 0xAA).all() and (m == 0xAAAAAAAA).all() and (ln == 0xAAAAAAAA).all()
    assert engine.qp_clean_batch([]) [0] == []
    assert engine.remove_quoted_printable_soft_breaks(b"ab=\r\ncd=") == (b"abcd=\0\0\0", [0, 1, 5, 6, 7] + [2 ** 64 - 1] * 3)


# ---- zke_extract_captures_mapped
MARK, TAIL, LAST = r"MARK-([0-9]*);", r"TAIL([^x]*)", r"END\r\n()"
BODY_PARTS = [(MARK, [0, 1]), (TAIL, [1]), (LAST, [1])]
FILL = [b"The quick brown fox jumps over the lazy dog, again and again.", b"lorem ipsum dolor sit amet consectetur adipiscing elit sed do",
        b"one  two   three \t ", b"pack my box with five dozen liquor jugs"]


def body_of(kind: int, k: int) -> bytes:
    """A 64..512-byte body with one MARK-...; and TAIL-END as its last line; `kind` picks where the soft breaks sit."""
    mark = {0: b"MARK-12345678;",                       # no break anywhere near
            1: b"MARK-1234=\r\n5678;",                   # a break inside group 1 (SPLIT)
            2: b"=\r\nMARK-12345678;=\r\n",              # breaks directly in front of and behind the match (no flag, shifted by 3)
            3: b"MARK-;",                                # an empty group
            4: b"=\r\n=\r\nMA=\r\nRK-=\r\n1=\r\n=\r\n2;=\r\n"}[kind]     # runs, a break between "-" and the group, and inside it
    lines = [FILL[(k + j) % len(FILL)] for j in range(1 + k % 5)]
    pre = b"\r\n".join(lines[:1 + k % 2]) + (b"" if kind in (2, 4) else b"\r\n")
    post = b"\r\n" + b"\r\n".join(lines[1 + k % 2:] + [b"soft=", b"ened"] * (k % 3 == 1) + [b"TAIL-END"]) + b"\r\n"
    return pre + b"pad " * (k % 7) + mark + post


def make_emails(n, seed=5):
    """(emails, canonical haystacks or None where the e-mail fails) — both body canonicalisations, with and without l=, one e-mail
    that fails DKIM and one that matches MARK twice."""
    rng = np.random.default_rng(seed)
    key = synth.keys_of(2048, 1)[0]
    emails, hays = [], []
    for i in range(n):
        body = body_of(i % 5, i)
        relaxed = bool((i // 5) % 2)
        fail = {7: "dkim", 11: "count"}.get(i)
        if fail == "count":
            body = b"MARK-1;\r\n" + body
        core = synth.relaxed_body(body) if relaxed else synth.simple_body(body)
        spec = synth.SignSpec(domain="example.com", body_canon="relaxed" if relaxed else "simple")
        if (i // 10) % 2:                               # l=: the signed body ends where `body` ends, a trailer follows
            spec.length = len(core)
            body = body + b"unsigned trailer  line\r\n\r\n"
        raw, it = synth.sign_email(synth.std_headers(rng, i, "example.com"), body, key, spec, corrupt="body" if fail == "dkim" else None)
        emails.append(A.Email("example.com", raw, A.PublicKey(key.pkcs1_der, "rsa")))
        hays.append(None if fail else (body, relaxed, spec.length))
    return emails, hays


def run_extract(engine, emails, parts, n_header, mapped, asynchronous=False):
    """zke_extract_captures[_mapped][_async] with explicit (dfa id, program id, groups) per part; returns a dict of everything delivered,
    or (after submission) the pending call's state when `asynchronous`."""
    arr = (A.zke_capture_part * len(parts))()
    keep = [np.array(g, np.uint32) for _, _, g in parts]
    for k, (d, p, g) in enumerate(parts):
        arr[k].dfa_id, arr[k].prog_id, arr[k].n_groups, arr[k].groups = d, p, len(g), keep[k].ctypes.data
    refs = A.EmailRefs(emails)
    n, P, G = refs.n, len(parts), sum(len(g) for _, _, g in parts)
    st = dict(n=n, G=G, out=np.zeros(max(n, 1), dtype=A.RESULT_DTYPE), spans=np.zeros(max(n * G * 2, 1), np.uint32), flags=np.zeros(max(n * G, 1), np.uint8),
              cap_off=np.zeros(n * P + 1, np.uint32), cap_str_off=np.zeros(n * G + 1, np.uint32), blob=np.zeros(max(64 * n * G, 1), np.uint8),
              ospans=np.full(max(n * G * 2, 1), 0x55555555, np.uint32), oflags=np.full(max(n * G, 1), 0x55, np.uint8), keep=(arr, keep, refs))
    o = A.zke_capture_out()
    o.spans, o.spans_cap, o.flags, o.flags_cap = st["spans"].ctypes.data, n * G * 2, st["flags"].ctypes.data, n * G
    o.cap_off, o.cap_off_cap, o.cap_str_off, o.cap_str_off_cap = st["cap_off"].ctypes.data, n * P + 1, st["cap_str_off"].ctypes.data, n * G + 1
    o.cap_blob, o.cap_blob_cap = st["blob"].ctypes.data, 64 * n * G
    org = A.zke_capture_origin()
    org.spans, org.spans_cap, org.flags, org.flags_cap = st["ospans"].ctypes.data, n * G * 2, st["oflags"].ctypes.data, n * G
    st["o"], st["org"] = o, org
    body = C.cast(C.byref(arr, n_header * C.sizeof(A.zke_capture_part)), C.POINTER(A.zke_capture_part))
    args = [engine.h, refs.arr, n, arr, n_header, body, P - n_header, st["out"].ctypes.data, C.byref(o)] + ([C.byref(org)] if mapped else [])
    name = "zke_extract_captures" + ("_mapped" if mapped else "") + ("_async" if asynchronous else "")
    if asynchronous:
        st["ticket"] = C.c_uint64()
        args.append(C.byref(st["ticket"]))
    assert getattr(engine.lib, name)(*args) == 0, engine.lib.zke_last_error(None)
    return st


def delivered(st):
    n, G = st["n"], st["G"]
    return dict(out=st["out"][:n].tobytes(), spans=st["spans"][:n * G * 2].tolist(), flags=st["flags"][:n * G].tolist(), cap_off=st["cap_off"].tolist(),
                cap_str_off=st["cap_str_off"][:int(st["o"].n_strings) + 1].tolist(), blob=st["blob"][:int(st["o"].cap_blob_need)].tobytes())


def parts_of(engine, patterns):
    out = []
    for pat, groups in patterns:
        _, dfa_id, prog_id = engine.compile_pattern(pat, False)
        assert engine.dfa_status(dfa_id) == 0 and engine.capture_status(prog_id) == 0, pat
        out.append((dfa_id, prog_id, groups))
    return out


def expected_origins(oracle, hay, patterns):
    """Per requested group of the body parts: (span, origin + flags) by the model on the oracle's canonical body, truncated as the
    verify pass truncates it, the span found with `re` in the cleaned, zero-padded haystack."""
    body, relaxed, length = hay
    canon = oracle.canon_body(body, relaxed)
    if length is not None:
        canon = canon[:length]
    cleaned, im, kept = Q.remove_qp(canon)
    out = []
    for pat, groups in patterns:
        ms = list(re.finditer(pat.encode(), cleaned, flags=re.S))
        assert len(ms) == 1, (pat, canon)
        for g in groups:
            s, e = ms[0].span(g)
            out.append(((s, e), Q.origin(im, len(canon), s, e)))
    return out, canon, cleaned


@pytest.fixture(scope="module")
def signed():
    return make_emails(65)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_origins_through_extraction(engine, oracle, signed, n):
    emails, hays = signed[0][:n], signed[1][:n]
    hdr = [(p, ci) for p, ci in synth.HEADER_PATTERNS]
    st = run_extract(engine, emails, parts_of(engine, hdr + BODY_PARTS), len(hdr), mapped=True)
    G, gh = st["G"], sum(len(g) for _, g in hdr)
    spans, ospans, oflags = st["spans"][:n * G * 2].reshape(n, G, 2), st["ospans"][:n * G * 2].reshape(n, G, 2), st["oflags"][:n * G].reshape(n, G)
    seen = set()
    for i in range(n):
        if hays[i] is None:                                               # fails DKIM / its match count: no strings, the pair stands
            assert st["out"][i]["status"] != A.ZKE_OK and (spans[i] == NO).all() and (ospans[i] == NO).all() and not oflags[i].any(), i
            continue
        assert st["out"][i]["status"] == A.ZKE_OK, (i, st["out"][i]["status"], st["out"][i]["detail"])
        assert (ospans[i, :gh] == spans[i, :gh]).all() and not oflags[i, :gh].any() and (spans[i, :gh] != NO).all(), i      # header parts: identity
        want, canon, cleaned = expected_origins(oracle, hays[i], BODY_PARTS)
        for c, ((s, e), (os_, oe, fl)) in enumerate(want):
            got = (tuple(int(x) for x in spans[i, gh + c]), (int(ospans[i, gh + c, 0]), int(ospans[i, gh + c, 1]), int(oflags[i, gh + c])))
            assert got == ((s, e), (os_, oe, fl)), (i, c, canon)
            if fl == 0:
                assert canon[os_:oe] == cleaned[s:e]
            seen.add((c, fl, e == s))
    if n >= 63:
        # a break inside a capture; an empty group; a group at clean_len; one that runs into the padding through [^x]*; and the same without
        assert {(1, Q.ORGF_SPLIT, False), (0, Q.ORGF_SPLIT, False), (1, 0, True), (3, Q.ORGF_PADDING, True), (2, Q.ORGF_PADDING, False), (2, 0, False),
                (0, 0, False)} <= seen, seen
        i = next(k for k in range(n) if k % 5 == 2 and hays[k] is not None)     # breaks right in front of and behind the match: shifted, no flag
        gs, ge = spans[i, gh]
        assert int(oflags[i, gh]) == 0 and (int(ospans[i, gh, 0]) - int(gs)) % 3 == 0 and int(ospans[i, gh, 0]) > int(gs)
        assert int(ospans[i, gh, 1]) - int(ospans[i, gh, 0]) == int(ge) - int(gs)
        assert any(h is None for h in hays)
    # the Python keyword delivers the same
    cfg = rc.RegexConfig([rc.RegexPattern(p, ci) for p, ci in hdr], [rc.RegexPattern(p, ci) for p, ci in BODY_PARTS])
    recs, infos, (os2, of2) = engine.extract_captures(emails, cfg, unicode=False, origins=True)
    assert recs.tobytes() == st["out"][:n].tobytes() and (os2 == ospans).all() and (of2 == oflags).all()
    assert len(engine.extract_captures(emails[:1], cfg, unicode=False)) == 2
    if n == 1:
        check_16_parts_of_16_groups(engine, oracle)


def check_16_parts_of_16_groups(engine, oracle):
    """512 queries on one e-mail: every lane of the wave holds eight, the breaks fall between and inside the groups."""
    pat = "Q" + "([0-9])" * 15 + ";"
    body = b"first line of the body\r\nQ12=\r\n345=\r\n=\r\n6789012=\r\n345;=\r\n tail\r\n"
    key = synth.keys_of(2048, 1)[0]
    raw, it = synth.sign_email(synth.std_headers(np.random.default_rng(1), 0, "example.com"), body, key, synth.SignSpec(domain="example.com"))
    patterns = [(pat, list(range(16)))] * 16
    st = run_extract(engine, [A.Email("example.com", raw, A.PublicKey(key.pkcs1_der, "rsa"))], parts_of(engine, patterns), 0, mapped=True)
    assert st["out"][0]["status"] == A.ZKE_OK and st["G"] == 256
    want, canon, cleaned = expected_origins(oracle, (body, True, None), patterns)
    got = [((int(a), int(b)), (int(c), int(d), int(f))) for (a, b), (c, d), f in
           zip(st["spans"].reshape(256, 2), st["ospans"].reshape(256, 2), st["oflags"])]
    assert got == want
    assert {f for _, (_, _, f) in want} == {0, Q.ORGF_SPLIT}


def test_mapped_equals_plain(signed):
    """Records, spans, flags, tables and blob of the mapped extraction are those of the plain one; the asynchronous form through three
    slots, a header-only batch (no origin launch: the origins are the spans) among them."""
    eng = z.Engine(slots=3)
    try:
        emails = signed[0]
        hdr = [(p, ci) for p, ci in synth.HEADER_PATTERNS]
        full, honly = parts_of(eng, hdr + BODY_PARTS), parts_of(eng, hdr)
        chunks = [(emails[:20], full, 2), (emails[20:41], honly, 2), (emails[41:65], full, 2), (emails[5:30], full, 2), (emails[:1], full, 2)]
        plain = [delivered(run_extract(eng, em, parts, nh, mapped=False)) for em, parts, nh in chunks]
        sync = [run_extract(eng, em, parts, nh, mapped=True) for em, parts, nh in chunks]
        pend = [run_extract(eng, em, parts, nh, mapped=True, asynchronous=True) for em, parts, nh in chunks]      # five batches over three slots
        for st in pend:
            assert eng.lib.zke_batch_wait(eng.h, st["ticket"]) == 0
        for p, s, a, (em, parts, nh) in zip(plain, sync, pend, chunks):
            assert delivered(s) == p and delivered(a) == p
            n, G = s["n"], s["G"]
            assert a["ospans"][:n * G * 2].tolist() == s["ospans"][:n * G * 2].tolist() and a["oflags"][:n * G].tolist() == s["oflags"][:n * G].tolist()
            if parts is honly:
                assert s["ospans"][:n * G * 2].tolist() == p["spans"] and not s["oflags"][:n * G].any()
    finally:
        eng.close()


def test_cpp_mirror(tmp_path, oracle):
    exe = build.build_cpp_qpmap()
    body = b"ab=\r\ncd=\r\n=\r\nef" + b"g" * 60 + b"=\r\nh="
    cleaned, im, kept = Q.remove_qp(body)
    (tmp_path / "body.bin").write_bytes(body)
    mail = body_of(1, 3)
    key = synth.keys_of(2048, 1)[0]
    raw, it = synth.sign_email(synth.std_headers(np.random.default_rng(2), 0, "example.com"), mail, key, synth.SignSpec(domain="example.com"))
    dfa = rc.create_dfa(MARK, unicode=False)
    for name, data in (("m.eml", raw), ("key.der", key.pkcs1_der), ("fwd", dfa.fwd), ("bwd", dfa.bwd), ("prog", rc.create_capture_program(MARK, unicode=False))):
        (tmp_path / name).write_bytes(data)
    r = subprocess.run([exe, str(tmp_path / "body.bin")] + [str(tmp_path / f) for f in ("m.eml",)] + ["example.com"] +
                       [str(tmp_path / f) for f in ("key.der", "fwd", "bwd", "prog")] + ["0", "1"], capture_output=True, text=True, timeout=120)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert lines[0] == "QP %d %s" % (kept, cleaned.hex())
    assert lines[1] == "MAP " + " ".join("MAX" if x == Q.NO_INDEX else str(x) for x in im)
    want, canon, _ = expected_origins(oracle, (mail, True, None), [(MARK, [0, 1])])
    assert lines[2] == "REC 0 0"
    assert lines[3:5] == ["ORG %d %d %d %d %d" % (s, e, a, b, f) for (s, e), (a, b, f) in want]
    assert want[1][1][2] == Q.ORGF_SPLIT and lines[5] == "SAME 1"
