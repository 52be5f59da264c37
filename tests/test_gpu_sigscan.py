"""-m gpu: zke_scan_signatures and zke_select_keys (helpers/src/generator.rs:11-53 around the caller's DNS fetch) against the
models of tests/sigscan_model.py — every record of every e-mail, none excluded — and against the verify path itself; the chain
generate_email_inputs -> generate_email_with_regex_inputs -> verify_emails_with_regex; re-entrancy from four host threads."""
import ctypes as C
import threading

import numpy as np
import pytest

import zkemail_rs_amd as z
from zkemail_rs_amd import _abi as A

import cases
import sigscan_inputs as I
import sigscan_model as M
import strict_cases as S
import synth
from test_gpu_verify import assert_records_equal, more_seeds

pytestmark = pytest.mark.gpu


def assert_scans_equal(got, exp, pairs, ctx):
    """status, detail, both counts and every record's header_index, code, algo, selector bytes and value span."""
    assert len(got) == len(exp)
    for i, (g, x) in enumerate(zip(got, exp)):
        where = f"{ctx} e-mail {i}: engine {g.status}/{g.detail} model {x.status}/{x.detail}; head {pairs[i][0][:120]!r}"
        assert (g.status, g.detail, g.n_signatures, g.n_candidates) == (x.status, x.detail, x.n_signatures, x.n_candidates), where
        assert len(g.sigs) == len(x.sigs), where
        for k, (a, b) in enumerate(zip(g.sigs, x.sigs)):
            assert tuple(a) == tuple(b), f"{where}; record {k}: engine {a} model {b}"


def scan_both(engine, pairs, max_sigs=8, **kw):
    raws, doms = [p[0] for p in pairs], [p[1] for p in pairs]
    return engine.scan_signatures(raws, doms, max_sigs), M.scan(raws, doms, max_sigs, **kw)


def test_scan_parity_corpus_and_limit_cases(engine):
    """The whole corpus, the limit cases (250 headers, the 63 / 64 / 65 filler boundary of the LDS span table, a 14 KB header
    block, 300 headers) and e-mails with up to 21 signatures; every code the scan can give is met."""
    names, pairs, cs = I.corpus()
    for ms in (64, 8):
        got, exp = scan_both(engine, pairs, ms)
        assert_scans_equal(got, exp, pairs, f"corpus max_sigs={ms}")
    codes = {s.code for g in got for s in g.sigs}
    assert {0, A.D_NEUTRAL, A.D_FROM_NOT_SIGNED, A.D_DOMAIN_MISMATCH, A.D_BAD_QUERY_METHOD, A.D_INCOMPATIBLE_VERSION, A.D_MISSING_TAG,
            A.D_SIG_SYNTAX, A.D_U_SIG_NON_ASCII, A.D_U_TOO_MANY_TAGS, A.D_U_SIG_TOO_LONG} <= codes
    by_name = dict(zip(names, got))
    assert (by_name["unsupported_300_headers"].status, by_name["unsupported_300_headers"].detail) == (A.ZKE_UNSUPPORTED, A.D_U_TOO_MANY_HEADERS)
    assert (by_name["unsupported_from_domain_kelvin_sign"].status, by_name["unsupported_from_domain_kelvin_sign"].detail) == (A.ZKE_UNSUPPORTED, A.D_U_DOMAIN_FOLD)
    assert by_name["pass_250_headers"].n_candidates == 1 and by_name["pass_after_20_failed_signatures"].n_signatures == 21
    for c, g in zip(cs, got):
        if c.status == A.ZKE_PARSE_FAIL:
            assert g.status == A.ZKE_PARSE_FAIL and not g.sigs, c.name


def test_scan_parity_taglist_fuzz(engine):
    pairs, kinds, _ = I.taglist_headers()
    assert len(pairs) == 4096
    got, exp = scan_both(engine, pairs)
    assert_scans_equal(got, exp, pairs, "tag-list fuzz")
    assert sum(g.n_candidates for g in got) > 2500


def test_scan_parity_mime_fuzz(engine):
    pairs = I.mime_fuzz_emails()
    assert len(pairs) == 1536
    got, exp = scan_both(engine, pairs)
    assert_scans_equal(got, exp, pairs, "MIME fuzz")
    seen = {(g.status, g.detail) for g in got}
    assert (A.ZKE_OK, 0) in seen and (A.ZKE_PARSE_FAIL, A.D_SUBPART_LEADING_SPACE) in seen and (A.ZKE_UNSUPPORTED, A.D_U_MIME_CTYPE) in seen


@pytest.mark.parametrize("seed", more_seeds([99, 7, 2026, 31337], first=7000))
def test_scan_parity_mutation_fuzz(engine, seed):
    """600 byte-mutated e-mails per seed (2 400 by default; ZKE_FUZZ_SEEDS adds seeds)."""
    pairs = I.mutation_fuzz_emails(seed)
    got, exp = scan_both(engine, pairs, 8)
    assert_scans_equal(got, exp, pairs, f"mutation fuzz seed {seed}")
    assert len({s.code for g in got for s in g.sigs}) >= 3


@pytest.mark.parametrize("max_sigs", [1, 8, 64])
def test_scan_signature_counts_around_max_sigs(engine, max_sigs):
    counts = sorted({0, 1, max(max_sigs - 1, 0), max_sigs, max_sigs + 1, 21})
    pairs = [I.email_with_signatures(c, seed=k) for k, c in enumerate(counts)]
    got, exp = scan_both(engine, pairs, max_sigs)
    assert_scans_equal(got, exp, pairs, f"max_sigs={max_sigs}")
    for c, g in zip(counts, got):
        assert g.n_signatures == c and len(g.sigs) == min(c, max_sigs)          # the list is cut, the counts are not


def test_scan_selector_lengths_empty_input_and_kelvin(engine):
    pairs, sels = I.selector_emails()
    got, exp = scan_both(engine, pairs)
    assert_scans_equal(got, exp, pairs, "selector lengths")
    assert [g.sigs[0].selector for g in got] == sels and all(g.sigs[0].code == 0 for g in got)
    assert engine.scan_signatures([], []) == []
    extra = [(b"", "example.com"), (b"", ""), (b"\r\n", "example.com"), (pairs[0][0], "example.\u212aom"), (pairs[0][0], "\u212a"),
             (pairs[0][0], ""), (b"DKIM-Signature", "example.com"), (b"DKIM-Signature:", "example.com"), (b"dkim-signature: v=1", "example.com")]
    got, exp = scan_both(engine, extra)
    assert_scans_equal(got, exp, extra, "edges")
    assert (got[3].status, got[3].detail) == (A.ZKE_UNSUPPORTED, A.D_U_DOMAIN_FOLD) and got[0].n_signatures == 0


@pytest.mark.parametrize("flags", [dict(enforce_expiry_x=1), dict(i_must_be_subdomain=1), dict(enforce_expiry_x=1, i_must_be_subdomain=1)])
def test_scan_applies_the_strictness_flags(flags):
    eng = z.Engine(now_unix=S.NOW, **flags)
    try:
        pairs = [(c[2].raw_email, c[2].from_domain) for c in S.plain_cases()]
        got, exp = scan_both(eng, pairs, strict=A.strict_mask(**flags), now=S.NOW)
        assert_scans_equal(got, exp, pairs, str(flags))
        assert {s.code for g in got for s in g.sigs} >= {0, A.D_SIG_EXPIRED if "enforce_expiry_x" in flags else A.D_DOMAIN_MISMATCH}
    finally:
        eng.close()


def test_scan_agrees_with_the_verify_path(engine):
    """No model involved: an e-mail zke_verify_emails reports ZKE_OK with sig_index j has a candidate as its j-th record; an e-mail
    whose scan has no candidate is ZKE_DKIM_NOT_PASS / ZKE_D_NEUTRAL, a key failure or a parse failure on the verify path."""
    names, pairs, cs = I.corpus()
    recs = engine.verify_emails([c.email for c in cs])
    scans = engine.scan_signatures([p[0] for p in pairs], [p[1] for p in pairs], 64)
    n_ok = 0
    for nm, r, sc in zip(names, recs, scans):
        if int(r["status"]) == A.ZKE_OK:
            n_ok += 1
            assert sc.status == A.ZKE_OK and sc.sigs[int(r["sig_index"])].code == 0, nm
        if sc.status == A.ZKE_OK and sc.n_candidates == 0:
            assert (int(r["status"]), int(r["detail"])) == (A.ZKE_DKIM_NOT_PASS, A.D_NEUTRAL) or int(r["status"]) in (A.ZKE_KEY_DECODE_FAIL, A.ZKE_UNSUPPORTED) or \
                   (int(r["status"]) == A.ZKE_DKIM_NOT_PASS and int(r["detail"]) in [s.code for s in sc.sigs]), (nm, int(r["status"]), int(r["detail"]))
        if sc.status != A.ZKE_OK and int(r["status"]) != A.ZKE_KEY_DECODE_FAIL:
            assert (int(r["status"]), int(r["detail"])) == (sc.status, sc.detail), nm
    assert n_ok > 60


def test_scan_blob_too_small(engine):
    """ZKE_E_NOMEM, the fixed-size outputs delivered, sel_blob_need exact; the second call succeeds."""
    pairs = [I.email_with_signatures(c, seed=c) for c in (3, 0, 7, 1)] + I.selector_emails()[0]
    refs = engine._scan_refs([p[0] for p in pairs], [p[1] for p in pairs])
    exp = M.scan([p[0] for p in pairs], [p[1] for p in pairs], 8)
    need = sum(len(s.selector) for x in exp for s in x.sigs)
    from zkemail_rs_amd.engine import _ScanBuffers
    for cap in (0, 5, need - 1):
        b = _ScanBuffers(refs.n, 8, cap)
        rc = engine.lib.zke_scan_signatures(engine.h, refs.arr, refs.n, 8, C.byref(b.c))
        assert rc == -3 and int(b.c.sel_blob_need) == need and int(b.c.n_sigs) == sum(len(x.sigs) for x in exp), (cap, rc)
        for i, x in enumerate(exp):
            assert tuple(int(v) for v in b.status[i]) == (x.status, x.detail, x.n_signatures, x.n_candidates)
            rows = b.sigs[int(b.sig_off[i]):int(b.sig_off[i + 1])]
            assert [(int(r["header_index"]), int(r["code"]), int(r["algo"]), int(r["sel_len"]), (int(r["val_start"]), int(r["val_end"]))) for r in rows] == \
                   [(s.header_index, s.code, s.algo, len(s.selector), s.value_span) for s in x.sigs]
    b = _ScanBuffers(refs.n, 8, need)
    assert engine.lib.zke_scan_signatures(engine.h, refs.arr, refs.n, 8, C.byref(b.c)) == 0
    assert_scans_equal(b.result(), exp, pairs, "exact blob")
    # a record buffer that is too small: refused at once when its size is known up front, reported with sigs_need otherwise
    b = _ScanBuffers(refs.n, 8, need)
    b.c.sigs_cap = 2
    assert engine.lib.zke_scan_signatures(engine.h, refs.arr, refs.n, 8, C.byref(b.c)) == -3 and int(b.c.sigs_need) == sum(len(x.sigs) for x in exp)
    b.c.sig_off_cap = refs.n
    assert engine.lib.zke_scan_signatures(engine.h, refs.arr, refs.n, 8, C.byref(b.c)) == -3
    assert engine.lib.zke_scan_signatures(engine.h, refs.arr, refs.n, 0, C.byref(b.c)) == -1
    assert engine.lib.zke_scan_signatures(engine.h, refs.arr, refs.n, 65, C.byref(b.c)) == -1


# ---- selection
def _wrong_keys():
    ed = cases.ED()
    return [A.PublicKey(cases.K("rsa2048_01").pkcs1_der), None, A.PublicKey(b""), A.PublicKey(b"\x30\x03\x02\x01"), A.PublicKey(b"garbage" * 9),
            A.PublicKey(ed[0].pub, "ed25519"), A.PublicKey(ed[1].pub[:31], "ed25519"), A.PublicKey(cases.K("rsa1024_00").pkcs1_der),
            A.PublicKey(cases.K("rsa2048_00").pkcs1_der, "dsa")]


def test_select_keys_against_the_model():
    """Multi-signature e-mails with up to 20 candidates, the passing key in every position, failed fetches, undecodable DER, an
    Ed25519 key against RSA signatures and the reverse, e-mails without candidates: chosen and the whole record as the model has
    them, and the record identical to zke_verify_emails of the e-mail with the chosen key.  The e-mail with 20 same-domain
    signatures needs 20 signature rounds: the engine is made with max_sig_rounds=32 (the default cap of 16 reports such an e-mail
    as ZKE_UNSUPPORTED / ZKE_D_U_TOO_MANY_SIGS, which the last lines check on a default engine)."""
    engine = z.Engine(max_sig_rounds=32)
    try:
        _select_keys_against_the_model(engine)
    finally:
        engine.close()
    dflt = z.Engine()
    try:
        c = cases.multi_signature_case(19)
        recs, chosen = dflt.select_keys([c.email], [[c.email.public_key]])
        assert int(chosen[0]) == A.SEL_NONE and (int(recs[0]["status"]), int(recs[0]["detail"])) == (A.ZKE_UNSUPPORTED, A.D_U_TOO_MANY_SIGS)
    finally:
        dflt.close()


def _select_keys_against_the_model(engine):
    rng = np.random.default_rng(8)
    wrong = _wrong_keys()
    emails, cands = [], []
    for n_bad in (0, 1, 3, 19):
        c = cases.multi_signature_case(n_bad)
        right = c.email.public_key
        for pos in range(n_bad + 1):                         # the passing key in every position
            row = [wrong[int(rng.integers(0, len(wrong)))] for _ in range(n_bad + 1)]
            row[pos] = right
            emails.append(c.email)
            cands.append(row)
        emails.append(c.email); cands.append([wrong[int(rng.integers(0, len(wrong)))] for _ in range(n_bad + 1)])     # nothing passes
        emails.append(c.email); cands.append([])                                                                       # no candidate
    ed_case = [c for c in cases.build_cases() if c.name == "pass_ed25519_relaxed_relaxed"][0]                        # the reverse: RSA keys against an Ed25519 signature
    emails += [ed_case.email] * 3
    cands += [[wrong[0], ed_case.email.public_key], [ed_case.email.public_key], [wrong[0], wrong[7]]]
    c3 = cases.multi_signature_case(3)
    emails.append(c3.email)
    cands.append([wrong[0], None, wrong[5], c3.email.public_key, c3.email.public_key])
    recs, chosen = engine.select_keys(emails, cands)
    xrecs, xchosen = M.select_keys(emails, cands)
    assert [int(v) for v in chosen] == [int(v) for v in xchosen]
    assert_records_equal(recs, xrecs, None, "select_keys")
    assert int(chosen[-1]) == 3 | A.SEL_AFTER_UNSUPPORTED
    assert A.SEL_NONE in [int(v) for v in chosen] and 19 in [int(v) & 0x7FFFFFFF for v in chosen]
    # the record is zke_verify_emails' of the e-mail with the chosen key, all 192 bytes
    picked = [(e, row[int(ch) & 0x7FFFFFFF], r) for e, row, ch, r in zip(emails, cands, chosen, recs) if int(ch) != A.SEL_NONE]
    direct = engine.verify_emails([A.Email(e.from_domain, e.raw_email, k, e.external_inputs) for e, k, _ in picked])
    for (e, k, r), d in zip(picked, direct):
        assert r.tobytes() == d.tobytes()
    none = [r for ch, row, r in zip(chosen, cands, recs) if not row]
    assert none and all(r.tobytes() == none[0].tobytes() and int(r["status"]) == A.ZKE_DKIM_NOT_PASS and int(r["detail"]) == A.D_NEUTRAL and
                        not any(r["from_domain_hash"]) for r in none)
    # nothing to select from at all, and a cand_off that goes down
    r0, c0 = engine.select_keys(emails[:3], [[], [], []])
    assert [int(v) for v in c0] == [A.SEL_NONE] * 3 and all(int(s) == A.ZKE_DKIM_NOT_PASS for s in r0["status"])
    assert engine.select_keys([], [])[1].size == 0
    refs = A.EmailRefs(emails[:2])
    off = np.array([2, 1, 3], np.uint32)
    keys = (A.zke_key_ref * 3)()
    out, ch = np.zeros(2, A.RESULT_DTYPE), np.zeros(2, np.uint32)
    assert engine.lib.zke_select_keys(engine.h, refs.arr, 2, off.ctypes.data, keys, out.ctypes.data, ch.ctypes.data) == -1


def test_generate_email_inputs_chain(engine):
    """generate_email_inputs with a dict as resolver over the seeded two-signature workload, then generate_email_with_regex_inputs,
    then verify_emails_with_regex: every signed e-mail ends ZKE_OK; an unsigned one raises at its index."""
    from zkemail_rs_amd import regex_compile as rc
    doms, raws, resolver, unsigned = I.chain_workload()
    assert len(raws) == 1024 and 3 <= len(unsigned) <= 30
    calls = []

    def fetch(domain, selector):
        calls.append((domain, selector))
        return resolver.get((domain, selector))
    signed = [i for i in range(len(raws)) if i not in set(unsigned)]
    ext = [[A.ExternalInput("k", str(i), 8)] for i in signed]
    emails = z.generate_email_inputs([doms[i] for i in signed], [raws[i] for i in signed], fetch, ext, engine=engine)
    assert len(calls) == len(set(calls)) == 16                       # once per distinct (domain, selector) pair
    for e, i in zip(emails, signed):
        assert e.raw_email == raws[i] and e.public_key.key == resolver[("example.com", b"key%02d" % (i % 16))].key and e.external_inputs[0].value == str(i)
    with pytest.raises(z.VerifyPanic) as ei:
        z.generate_email_inputs(doms, raws, fetch, engine=engine)
    assert ei.value.index == unsigned[0] and ei.value.reason == "No DKIM signatures found"
    sub = signed[:8]                                                   # a resolver that does not know one e-mail's key
    missing = b"key%02d" % (sub[2] % 16)
    with pytest.raises(z.VerifyPanic) as ei:
        z.generate_email_inputs([doms[i] for i in sub], [raws[i] for i in sub], lambda d, s: None if s == missing else resolver.get((d, s)), engine=engine)
    assert ei.value.index == 2 and ei.value.reason == "No valid DKIM key found for any signature" and ei.value.status == A.ZKE_DKIM_NOT_PASS
    with pytest.raises(z.VerifyPanic) as ei:
        z.generate_email_inputs(["example.com"], [b" leading space\r\n\r\n"], fetch, engine=engine)
    assert (ei.value.status, ei.value.detail) == (A.ZKE_PARSE_FAIL, A.D_HDR_LEADING_SPACE)
    cfg = rc.RegexConfig.from_json({"header_parts": [{"pattern": "s=(o[0-9]+);", "capture_indices": [1]}], "body_parts": None})
    with_regex = z.generate_email_with_regex_inputs(emails, cfg, engine=engine)
    recs = engine.verify_emails_with_regex(with_regex)
    assert (recs["status"] == A.ZKE_OK).all() and len(recs) == len(signed)
    # (canonicalize_signed_email takes the FIRST DKIM-Signature header, the foreign one: its selector is what the pattern finds)
    assert [w.regex_info.header_parts[0].captures for w in with_regex[:3]] == [["o%02d" % (i % 16)] for i in signed[:3]]


def test_scans_selections_and_verifications_from_four_threads():
    """Scans, selections and verifications from four host threads on a 3-slot engine (threads share slots), synchronous and
    asynchronous forms mixed: every result identical to a serial run on the same engine."""
    eng = z.Engine(slots=3, host_threads=4)
    try:
        names, pairs, cs = I.corpus()
        pairs = pairs[:60] + [I.email_with_signatures(c, seed=c) for c in (0, 1, 5, 9, 21)]
        raws, doms = [p[0] for p in pairs], [p[1] for p in pairs]
        c3 = cases.multi_signature_case(3)
        sel_emails = [c3.email] * 6 + [cs[0].email]
        wrong = _wrong_keys()
        sel_cands = [[wrong[k % len(wrong)], wrong[(k + 3) % len(wrong)], c3.email.public_key][:1 + k % 3] + ([c3.email.public_key] if k % 2 else []) for k in range(6)] + [[cs[0].email.public_key]]
        wl = synth.make_workload("mt", 80, 2500, rsa_bits=2048, n_keys=4, seed=91, ragged=True, invalid_frac=0.1)
        serial = {"scan8": eng.scan_signatures(raws, doms, 8), "scan64": eng.scan_signatures(raws, doms, 64),
                  "sel": eng.select_keys(sel_emails, sel_cands), "ver": eng.verify_emails(wl.emails)}
        errors = []

        def worker(t):
            try:
                for it in range(12):
                    kind = (t + it) % 4
                    if kind == 0:
                        assert eng.scan_signatures(raws, doms, 8) == serial["scan8"]
                    elif kind == 1:
                        ticket, pend = eng.scan_signatures_async(raws, doms, 64)
                        r2 = eng.verify_emails(wl.emails)
                        eng.wait(ticket)
                        assert pend.result() == serial["scan64"] and r2.tobytes() == serial["ver"].tobytes()
                    elif kind == 2:
                        ticket, r, ch = eng.select_keys_async(sel_emails, sel_cands)
                        eng.wait(ticket)
                        assert r.tobytes() == serial["sel"][0].tobytes() and list(ch) == list(serial["sel"][1])
                    else:
                        assert eng.verify_emails(wl.emails).tobytes() == serial["ver"].tobytes()
            except BaseException as ex:          # noqa: BLE001 — reported by the main thread
                errors.append((t, repr(ex)))
        ths = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        assert not errors, errors[:2]
        assert_scans_equal(serial["scan8"], M.scan(raws, doms, 8), pairs, "serial run")
    finally:
        eng.close()
