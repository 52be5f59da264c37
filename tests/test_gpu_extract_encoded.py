"""GPU: zke_extract_captures_encoded — extraction, String::from_utf8_lossy, the encode plan, abi_encode and SHA-256 in one batch
(csrc/capture_lossy.hip.h, csrc/utf8_lossy.hip.h, csrc/encode.hip.h) — on signed e-mails whose header and body carry crafted bytes,
patterns compiled in byte mode so that groups capture ill-formed UTF-8.
  * composition: records, spans, flags, cap_off equal zke_extract_captures' on the same batch; the strings equal its strings after
    Python's decode("utf-8", "replace"); the encodings equal abi_encode.py of the record's hashes, the external inputs and those
    strings; the digests equal hashlib.sha256 — every byte;
  * round trip: the delivered tables through zke_verify_emails_encoded (lists form, planned on the host) give the same records and,
    per e-mail, the same encoding and digest.  (The e-mail that fails on a missing group is left out there: the verify entry has no
    requested groups, so it cannot fail that way.  Groups are delimited by ASCII bytes, so the repaired capture is contained in the
    repaired match, which is what core/src/regex.rs:43-44 asks.)
  * the edges of the plan, short buffers, the asynchronous form, both DFA mappings, the refusal bound."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import synth
import utf8_lossy_cases as U
import zkemail_rs_amd as z
from zkemail_rs_amd import _abi as A
from zkemail_rs_amd import abi_encode as AE
from zkemail_rs_amd import regex_compile as rc

pytestmark = pytest.mark.gpu

E_ARG, E_NOMEM = -1, -3
ZERO32 = bytes(32)
GUARD = 64

# bytes a group can capture (no ">", CR, LF, "=", blank or tab: the body is canonicalised and QP-cleaned around them)
CRAFTED = [U.UNICODE_EXAMPLE, b"plain", b"", b"caf\xc3\xa9", "日本語".encode(), ("€" * 40).encode(), b"\xff", b"\x80\xbf", b"\xc0\x80",
           b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\xf0\x90\x80", b"a\xe2\x82", b"\xe2\x82\xacz\xbf", b"\xf0\x9f\x98\x80\xf0\x9f\x98",
           b"x" * 70 + b"\xf0\x9f\x98" + b"y" * 70, b"\xff" * 65]

CFG_MIX = rc.RegexConfig([rc.RegexPattern(r"subject:([^\r\n]+)\r\n", [1])],
                         [rc.RegexPattern(r"V<([^>]*)>", [0, 1]), rc.RegexPattern(r"G(a)|G(b)", [1])])


def key():
    return synth.keys_of(1024, 1)[0]


def sign(i, subject, body, fail=None, ext=None):
    rng = np.random.default_rng(1000 + i)
    hs = [(n, (subject if n == b"Subject" else v)) for n, v in synth.std_headers(rng, i, "example.com")]
    raw, _ = synth.sign_email(hs, body, key(), synth.SignSpec(domain="example.com"), corrupt="body" if fail == "dkim" else None)
    return A.Email("example.com", raw, A.PublicKey(key().pkcs1_der, "rsa"), ext or [])


def mix_emails(n=33, with_ext=True):
    """E-mails 0, n // 2 and n - 1 fail — bad signature, match count 2, missing group; the others carry CRAFTED bytes in the subject
    and in V<...>, and every third one external inputs."""
    out = []
    for i in range(n):
        c = CRAFTED[i % len(CRAFTED)]
        fail = {0: "dkim", n // 2: "count", n - 1: "group"}.get(i)
        body = b"line one\r\nV<" + c + b">\r\n" + (b"V<twice>\r\n" if fail == "count" else b"") + (b"Gb" if fail == "group" else b"Ga") + b"\r\nlast line\r\n"
        ext = [A.ExternalInput("addr", "0x%040x" % i), A.ExternalInput("né", "v" * (i % 40))] if with_ext and i % 3 == 0 else []
        out.append(sign(i, b"s" + CRAFTED[(i + 1) % len(CRAFTED)] + b"#%d" % i, body, fail, ext))
    return out


@pytest.fixture(scope="module")
def mix():
    return mix_emails()


def plain_extract(engine, r):
    """zke_extract_captures over the e-mails and parts of the call `r`: (records, spans, flags, cap_off, strings per e-mail)."""
    refs, arr, groups, _ = r.keep
    n, P, G = r.n, r.P, r.G
    nh = len(r.regex_config.header_parts or [])
    out = np.zeros(max(n, 1), dtype=A.RESULT_DTYPE)
    body = C.cast(C.byref(arr, nh * C.sizeof(A.zke_capture_part)), C.POINTER(A.zke_capture_part))
    call = lambda o: engine.lib.zke_extract_captures(engine.h, refs.arr, n, arr, nh, body, P - nh, out.ctypes.data, C.byref(o))
    rcode, spans, flags, cap_off, cap_str_off, blob = engine._run_captures(n, P, G, call, 64 * n * G)
    assert rcode == 0, engine.lib.zke_last_error(None)
    raw = blob.tobytes()
    strings = [[raw[int(cap_str_off[k]):int(cap_str_off[k + 1])] for k in range(int(cap_off[i * P]), int(cap_off[(i + 1) * P]))] for i in range(n)]
    return out[:n], spans, flags, cap_off, strings


def expected_encodings(records, emails, strings):
    out = []
    for rec, e, strs in zip(records, emails, strings):
        if rec["status"] != A.ZKE_OK:
            out.append((b"", ZERO32))
            continue
        ev = A.EmailVerifierOutput(rec["from_domain_hash"].tobytes(), rec["public_key_hash"].tobytes(), A.flat_external_inputs(e.external_inputs))
        enc = AE.abi_encode(ev, [s.decode("utf-8") for s in strs])
        out.append((enc, hashlib.sha256(enc).digest()))
    return out


ROOMY = dict(blob_bytes=1 << 16, bytes_cap=1 << 18)      # capacities no batch here comes near: one call suffices


def check_composition(engine, emails, cfg, r=None):
    """The whole delivery of one call against the composition of the parts; returns (the call, the expected (encoding, digest) list)."""
    if r is None:
        r = engine.extract_captures_encoded_call(emails, cfg, unicode=False, guard=GUARD, fill=0xAA, **ROOMY)
    assert r.rc == 0, engine.lib.zke_last_error(None)
    rec0, spans0, flags0, cap_off0, strings0 = plain_extract(engine, r)
    n, G = r.n, r.G
    assert r.records.tobytes() == rec0.tobytes()
    assert (r.spans[:n * G * 2].reshape(n, G, 2) == spans0).all() and (r.flags[:n * G].reshape(n, G) == flags0).all()
    assert (r.cap_off == cap_off0).all()
    want_strings = [[U.reference(s) for s in strs] for strs in strings0]
    assert r.strings() == want_strings
    total = sum(len(s) for strs in want_strings for s in strs)
    assert int(r.caps.cap_blob_need) == total and int(r.caps.n_strings) == sum(len(s) for s in want_strings)
    assert (r.blob[r.blob_bytes:] == 0xAA).all() and (r.blob[total:r.blob_bytes] == 0xAA).all(), "bytes behind the strings were written"
    want = expected_encodings(r.records, emails, want_strings)
    assert r.enc.result() == want
    # places: e-mails that are encoded follow each other without a gap; one that is not has no place
    at = 0
    for i, (enc, _) in enumerate(want):
        f = r.enc.infos[i]
        assert int(f["off"]) == at and int(f["len"]) == len(enc) and int(f["kind"]) == A.ENC_KIND_WITH_REGEX, i
        at += len(enc)
    assert int(r.enc.c.bytes_need) == at and int(r.enc.c.infos_need) == n
    assert (r.enc.bytes[at:] == 0xAA).all(), "bytes behind the encodings were written"
    return r, want


def test_composition_and_failures(engine, mix):
    r, want = check_composition(engine, mix, CFG_MIX)
    n = len(mix)
    st = [int(x) for x in r.records["status"]]
    assert st[0] != A.ZKE_OK and st[n // 2] == A.ZKE_BODY_REGEX_FAIL and st[n - 1] == A.ZKE_BODY_REGEX_FAIL
    assert int(r.records[n // 2]["detail"]) == A.D_RE_MATCH_COUNT and int(r.records[n - 1]["detail"]) == A.D_RE_GROUP_MISSING
    assert sum(s == A.ZKE_OK for s in st) == n - 3
    for i in (0, n // 2, n - 1):                 # len 0, a zero digest, no place: the next e-mail starts where this one would have
        assert want[i] == (b"", ZERO32) and int(r.enc.infos[i]["len"]) == 0
        if i + 1 < n:
            assert int(r.enc.infos[i + 1]["off"]) == int(r.enc.infos[i]["off"])
    assert sum(bool(f & A.CAPF_NOT_UTF8) for f in r.flags[:n * r.G]) >= 20 and r.strings() != plain_extract(engine, r)[4]
    # the Python mirror: one call, the strings as the device delivered them
    records, infos, encodings, digests = engine.extract_captures_encoded(mix, CFG_MIX, unicode=False)
    assert records.tobytes() == r.records.tobytes() and list(zip(encodings, digests)) == want
    assert [None if f is None else [c for p in (f.header_parts or []) + (f.body_parts or []) for c in p.captures] for f in infos] == \
           [None if s != A.ZKE_OK else [x.decode() for x in strs] for s, strs in zip(st, r.strings())]


def host_planned_round_trip(engine, r, emails):
    """The delivered records and tables through zke_encode_outputs — the host plan (encode_plan.hip.h) and the encode launch, no regex
    stage: per e-mail the same encoding and digest as the device-planned call gave."""
    outs = [A.EmailWithRegexVerifierOutput(A.EmailVerifierOutput(rec["from_domain_hash"].tobytes(), rec["public_key_hash"].tobytes(),
                                                                 A.flat_external_inputs(e.external_inputs)), [s.decode("utf-8") for s in strs])
            for rec, e, strs in zip(r.records, emails, r.strings())]
    enc = engine.encode_outputs(outs, [int(s) for s in r.records["status"]])
    assert enc.result() == r.enc.result()


def test_round_trip_through_the_host_planned_entries(engine, mix):
    r = engine.extract_captures_encoded_call(mix, CFG_MIX, unicode=False, **ROOMY)
    assert r.rc == 0
    host_planned_round_trip(engine, r, mix)
    # through zke_verify_emails_encoded (lists form): every e-mail the verify entry can judge as the extraction did — not the one that
    # fails on a missing group, and not those with a repaired string: the verify entry reports a capture that holds U+FFFD against a
    # match that is not UTF-8 as ZKE_UNSUPPORTED / ZKE_D_U_CAPTURE_FFFD (csrc/regex.hip.h) and does not compare them
    infos, got = r.regex_infos(), r.enc.result()
    flags = r.flags[:r.n * r.G].reshape(r.n, r.G)
    keep = [i for i in range(r.n) if int(r.records[i]["detail"]) != A.D_RE_GROUP_MISSING and not flags[i].any()]
    assert len(keep) >= 8 and any(int(r.records[i]["status"]) != A.ZKE_OK for i in keep)
    assert any(b > 0x7F for i in keep for s in r.strings()[i] for b in s)                       # (valid multi-byte strings among them)
    empty = A.RegexInfo([A.CompiledRegex(r.comp[0][0], [])], [A.CompiledRegex(r.comp[1][0], []), A.CompiledRegex(r.comp[2][0], [])])
    inputs = [A.EmailWithRegex(mix[i], infos[i] if infos[i] is not None else empty) for i in keep]
    records, encoded = engine.verify_emails_encoded(inputs, form="lists")
    assert records.tobytes() == r.records[keep].tobytes()
    assert encoded == [got[i] for i in keep]


def test_without_caps_and_without_external_inputs(engine, mix):
    full = engine.extract_captures_encoded_call(mix, CFG_MIX, unicode=False, **ROOMY)
    bare = engine.extract_captures_encoded_call(mix, CFG_MIX, unicode=False, want_caps=False, guard=GUARD, fill=0xAA, **ROOMY)
    assert full.rc == 0 and bare.rc == 0, engine.lib.zke_last_error(None)
    assert bare.records.tobytes() == full.records.tobytes() and bare.enc.result() == full.enc.result()
    assert (bare.blob == 0xAA).all() and not bare.spans.any() and not bare.cap_off.any()          # caps == NULL: nothing of it is touched
    noext = mix_emails(9, with_ext=False)
    r, want = check_composition(engine, noext, CFG_MIX)
    assert all(len(e.external_inputs) == 0 for e in noext) and sum(len(w[0]) > 0 for w in want) == 6


def test_zero_strings_and_more_than_64_strings(engine):
    # parts that request no group: every e-mail has zero strings, and is encoded with an empty matches array
    none = rc.RegexConfig(None, [rc.RegexPattern(r"V<([^>]*)>", []), rc.RegexPattern(r"G(a)|G(b)", [])])
    r, want = check_composition(engine, mix_emails(5), none)
    assert r.G == 0 and all(s == [] for s in r.strings()) and len(want[1][0]) == A.encoded_len(1, [], [])
    # five parts x ZKE_CAP_MAX_GROUPS single-byte groups: 80 strings per e-mail, across the encode kernel's 64-string pass
    dots = "(.)" * A.CAP_MAX_GROUPS
    wide = rc.RegexConfig(None, [rc.RegexPattern("Q%d=%s;" % (p, dots), list(range(1, A.CAP_MAX_GROUPS + 1))) for p in range(5)])
    alphabet = b"az09\xff\xc0\xf5\x80"                # every byte stands alone: ASCII, or one U+FFFD
    emails = []
    for i in range(4):
        rows = [bytes(alphabet[(i + 3 * p + 5 * k) % len(alphabet)] for k in range(A.CAP_MAX_GROUPS)) for p in range(5)]
        emails.append(sign(i, b"wide %d" % i, b"".join(b"Q%d=" % p + row + b";\r\n" for p, row in enumerate(rows))))
    r, want = check_composition(engine, emails, wide)
    assert all(len(s) == 80 for s in r.strings()) and all(len(w[0]) for w in want)
    host_planned_round_trip(engine, r, emails)


def test_repaired_lengths_0_31_32_33_and_three_times_the_span(engine):
    runs = [b"\xc3\xa9", b"\xc3\xa9\xc3\xa9" + b"\xff" * 9, b"\xc3\xa9" + b"\xff" * 10, b"\xff" * 11, b"\xff" * A.CAP_MAX_SPAN]
    cfg = rc.RegexConfig(None, [rc.RegexPattern(r"[^ -~\r\n]+", [0]), rc.RegexPattern(r"E<([a-z]*)>", [1])])
    emails = [sign(i, b"run %d" % i, b"E<" + (b"" if i % 2 == 0 else b"abc") + b">\r\nrun:" + run + b"\r\nend\r\n") for i, run in enumerate(runs)]
    r, want = check_composition(engine, emails, cfg)
    assert [[len(s) for s in strs] for strs in r.strings()] == [[2, 0], [31, 3], [32, 0], [33, 3], [3 * A.CAP_MAX_SPAN, 0]]
    assert all(int(x) == A.ZKE_OK for x in r.records["status"])


@pytest.mark.parametrize("which", ["bytes", "cap_blob"])
def test_short_buffer_reports_exact_needs(engine, mix, which):
    full = engine.extract_captures_encoded_call(mix, CFG_MIX, unicode=False, **ROOMY)
    assert full.rc == 0
    blob_need, bytes_need = int(full.caps.cap_blob_need), int(full.enc.c.bytes_need)
    for short in (0, 1, (bytes_need if which == "bytes" else blob_need) // 2, (bytes_need if which == "bytes" else blob_need) - 1):
        r = engine.extract_captures_encoded_call(mix, CFG_MIX, unicode=False, guard=GUARD, fill=0xAA,
                                                 bytes_cap=short if which == "bytes" else bytes_need,
                                                 blob_bytes=short if which == "cap_blob" else blob_need)
        assert r.rc == E_NOMEM
        assert int(r.caps.cap_blob_need) == blob_need and int(r.enc.c.bytes_need) == bytes_need and int(r.enc.c.infos_need) == r.n
        assert (r.blob[r.blob_bytes:] == 0xAA).all() and (r.enc.bytes[r.enc.nbytes:] == 0xAA).all(), "a byte beyond a capacity was written"
        assert r.records.tobytes() == full.records.tobytes()
        assert (r.spans == full.spans).all() and (r.flags == full.flags).all() and (r.cap_off == full.cap_off).all()
        assert (r.cap_str_off == full.cap_str_off).all()
        for i in range(r.n):                     # an e-mail is delivered whole, or reports len 0 and a zero digest at its planned place
            f, g = r.enc.infos[i], full.enc.infos[i]
            assert int(f["off"]) == int(g["off"])
            if int(f["len"]):
                assert r.enc.result()[i] == full.enc.result()[i] and int(f["off"]) + int(f["len"]) <= r.enc.nbytes
            else:
                assert f["digest"].tobytes() == ZERO32
        if which == "bytes":
            assert sum(int(f["len"]) > 0 for f in r.enc.infos[:r.n]) < sum(int(f["len"]) > 0 for f in full.enc.infos[:r.n])
    again = engine.extract_captures_encoded_call(mix, CFG_MIX, unicode=False, guard=GUARD, fill=0xAA, bytes_cap=bytes_need, blob_bytes=blob_need)
    check_composition(engine, mix, CFG_MIX, again)


def test_async_through_three_slots():
    eng = z.Engine(slots=3)
    batches = [mix_emails(7 + 4 * k) for k in range(3)]
    sync = [eng.extract_captures_encoded_call(b, CFG_MIX, unicode=False, **ROOMY) for b in batches]
    pend = [eng.extract_captures_encoded_call(b, CFG_MIX, unicode=False, ticket=True, **ROOMY) for b in batches]
    assert all(p.rc == 0 for p in pend) and all(s.rc == 0 for s in sync)
    for p, s in zip(reversed(pend), reversed(sync)):
        eng.wait(p.ticket)
        assert p.records.tobytes() == s.records.tobytes() and p.strings() == s.strings() and p.enc.result() == s.enc.result()
        assert (p.spans == s.spans).all() and (p.flags == s.flags).all() and (p.cap_off == s.cap_off).all()


@pytest.mark.parametrize("mapping", [1, 2])
def test_both_dfa_mappings(mix, mapping):
    eng = z.Engine(dfa_mapping=mapping)
    check_composition(eng, mix, CFG_MIX)


def test_refusals_before_staging(engine, mix):
    r = engine.extract_captures_encoded_call(mix[:2], CFG_MIX, unicode=False, **ROOMY)
    assert r.rc == 0
    refs, arr, groups, ext = r.keep
    body = C.cast(C.byref(arr, C.sizeof(A.zke_capture_part)), C.POINTER(A.zke_capture_part))
    call = lambda n, caps, enc, ext_off=None: engine.lib.zke_extract_captures_encoded(
        engine.h, refs.arr, n, arr, 1, body, 2, r.records.ctypes.data, caps, ext_off, ext.str_off.ctypes.data, ext.blob.ctypes.data, enc)
    # n * G * 3 * ZKE_CAP_MAX_SPAN >= 2^32: refused before an e-mail is read (the array holds two)
    n_bound = -(-2 ** 32 // (3 * A.CAP_MAX_SPAN * r.G))
    assert n_bound * r.G * 3 * A.CAP_MAX_SPAN >= 2 ** 32 > (n_bound - 1) * r.G * 3 * A.CAP_MAX_SPAN
    assert call(n_bound, None, C.byref(r.enc.c)) == E_ARG and b"3 * ZKE_CAP_MAX_SPAN" in engine.lib.zke_last_error(None)
    assert call(2, C.byref(r.caps), None) == E_ARG                                   # no zke_encoded_out
    small = A.EncodedBuffers(2, 4096)
    small.c.infos_cap = 1
    assert call(2, C.byref(r.caps), C.byref(small.c)) == E_NOMEM and int(small.c.infos_need) == 2
    bad = np.array([0, 2, 1], np.uint32)                                               # ext_off decreases
    assert call(2, C.byref(r.caps), C.byref(r.enc.c), bad.ctypes.data) == E_ARG
