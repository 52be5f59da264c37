"""-m gpu: zke_decode_key_records and zke_select_keys_from_records (helpers/src/dkim.rs:67-111 on the device) through the C-ABI
against the model of tests/keyrec_model.py — every record, none excluded: decode parity, the seeded mutation fuzz, the limits and
the buffer protocol, selection from records against selection from keys, the RFC 8463 message from its published records alone,
re-entrancy from four host threads."""
import ctypes as C
import threading

import numpy as np
import pytest

import zkemail_rs_amd as z
from zkemail_rs_amd import _abi as A
from zkemail_rs_amd.engine import _KeyrecBuffers

import cases
import keyrec_cases as K
import keyrec_model as M
import sigscan_inputs as I
import sigscan_model as SM
import synth

pytestmark = pytest.mark.gpu
MODES = (M.ARCHIVE, M.DNS)
E_ARG, E_NOMEM = -1, -3


def assert_keys_equal(got, exp, recs, ctx):
    """code, key type and every key byte."""
    assert len(got) == len(exp), ctx
    for i, (g, x) in enumerate(zip(got, exp)):
        assert (g.code, g.key_type, g.key) == (x.code, x.key_type, x.key), \
            f"{ctx} record {i}: engine {A.KEYREC_NAMES.get(g.code, g.code)}/{g.key_type}/{len(g.key)} bytes, model " \
            f"{A.KEYREC_NAMES.get(x.code, x.code)}/{x.key_type}/{len(x.key)} bytes; record {recs[i][:160]!r}"


@pytest.mark.parametrize("mode", MODES)
def test_decode_parity_fixture_keys_and_hand_cases(engine, mode):
    """Every fixture key as SubjectPublicKeyInfo and as PKCS#1, the Ed25519 keys, the RFC 8463 records, and ALL hand-written cases
    (those written for the other mode too: the model says what they give here)."""
    fx = K.fixture_records()
    recs = [r for _, r, _, _ in fx] + [c[2] for c in K.hand_cases()]
    got = engine.decode_key_records(recs, mode)
    assert_keys_equal(got, M.decode_all(recs, mode), recs, f"mode {mode}")
    for (name, _, kt, key), g in zip(fx, got):
        assert g.code == 0 and g.key_type == kt and (key is None or g.key == key), name
    for c, g in zip(K.hand_cases(), got[len(fx):]):            # the codes written down by hand, for the mode they were written for
        if c[1] == mode:
            assert (g.code, g.key_type, g.key) == (c[3], c[4], c[5]), c[0]


@pytest.mark.parametrize("mode", MODES)
def test_decode_mutation_fuzz(engine, mode):
    """4 096 seeded records: half one base64 character replaced inside p=, half structural.  No record is excused."""
    recs = K.fuzz_records(seed=100 + mode)
    assert len(recs) == 4096
    got = engine.decode_key_records(recs, mode)
    exp = M.decode_all(recs, mode)
    ok = sum(g.code == 0 for g in got)
    print(f"mode {mode}: {ok} of {len(got)} decode; codes {sorted({g.code for g in got})}")
    assert_keys_equal(got, exp, recs, f"fuzz mode {mode}")
    assert ok >= 1024 and len(got) - ok >= 1024, ok


@pytest.mark.parametrize("mode", MODES)
def test_decode_limits_and_buffer_protocol(engine, mode):
    lim = K.limit_records(mode)
    recs = [r for r, _, _ in lim]
    assert [len(r) for r in recs] == [A.KEYREC_MAX_BYTES - 1, A.KEYREC_MAX_BYTES, A.KEYREC_MAX_BYTES + 1]
    got = engine.decode_key_records(recs, mode)
    assert [(g.code, g.key) for g in got] == [(c, k) for _, c, k in lim]
    assert_keys_equal(got, M.decode_all(recs, mode), recs, "limits")
    # a batch of one, of none, and records that are "the fetch failed"
    assert_keys_equal(engine.decode_key_records(recs[:1], mode), M.decode_all(recs[:1], mode), recs, "one")
    assert engine.decode_key_records([], mode) == []
    assert [g.code for g in engine.decode_key_records([None, b"", recs[0]], mode)] == [A.D_KEYREC_NO_KEY, A.D_KEYREC_NO_KEY, 0]
    # every buffer one entry too small: ZKE_E_NOMEM, the needs exact, a second call succeeds
    mix = [r for _, r, _, _ in K.fixture_records()[:9]] + [b"v=DKIM1; p=!!!!", None]
    exp = M.decode_all([r or b"" for r in mix], mode)
    need = sum(len(x.key) for x in exp)
    b = _KeyrecBuffers(mix)
    b.c.infos_cap = len(mix) - 1
    assert engine.lib.zke_decode_key_records(engine.h, b.arr, b.m, mode, C.byref(b.c)) == E_NOMEM and int(b.c.infos_need) == len(mix)
    for cap in (0, need - 1):
        b = _KeyrecBuffers(mix, cap)
        assert engine.lib.zke_decode_key_records(engine.h, b.arr, b.m, mode, C.byref(b.c)) == E_NOMEM, cap
        assert (int(b.c.infos_need), int(b.c.keys_need)) == (len(mix), need)
        assert [(int(f["code"]), int(f["key_type"]), int(f["key_len"])) for f in b.infos] == [(x.code, x.key_type, len(x.key)) for x in exp]
    b = _KeyrecBuffers(mix, need)
    assert engine.lib.zke_decode_key_records(engine.h, b.arr, b.m, mode, C.byref(b.c)) == 0 and int(b.c.keys_need) == need
    assert_keys_equal(b.result(), exp, [r or b"" for r in mix], "exact buffer")
    assert engine.lib.zke_decode_key_records(engine.h, b.arr, b.m, 2, C.byref(b.c)) == E_ARG
    # the asynchronous form: the shortfall is reported by the wait
    b = _KeyrecBuffers(mix, need - 1)
    t = C.c_uint64()
    assert engine.lib.zke_decode_key_records_async(engine.h, b.arr, b.m, mode, C.byref(b.c), C.byref(t)) == 0
    assert engine.lib.zke_batch_wait(engine.h, t.value) == E_NOMEM and int(b.c.keys_need) == need
    ticket, pend = engine.decode_key_records_async(mix, mode)
    engine.wait(ticket)
    assert_keys_equal(pend.result(), exp, [r or b"" for r in mix], "async")


# ---- selection from records
def record_of(key, i=0):
    """A public key as a resolver would answer it: RSA keys as SubjectPublicKeyInfo or PKCS#1 in turn, in a few spellings (all of
    them read alike by both modes).  None stays None."""
    if key is None:
        return None
    if key.key_type == "ed25519":
        return b"v=DKIM1; k=ed25519; p=" + K.b64(key.key)
    if key.key_type != "rsa":
        return b"v=DKIM1; k=" + key.key_type.encode() + b"; p=" + K.b64(key.key)
    der = K.spki_wrap(key.key) if i % 3 != 2 else key.key
    return [b"v=DKIM1; k=rsa; p=", b"v=DKIM1; p=", b"k=rsa; p="][i % 3] + K.b64(der) + [b"", b";"][i % 2]


UNDECODABLE = [b"v=DKIM1; k=rsa; p=AAAA", b"v=DKIM1; k=rsa; p=", b"v=DKIM1; k=dsa; p=AAAA", b"v=DKIM1; k=ed25519; p=AAAA", b"k=rsa; p=A"]


def selection_batches():
    """The batches of tests/sigscan_inputs.py as (e-mails, candidate keys): the corpus with its multi-signature e-mails — every
    e-mail's own key behind as many wrong ones as it has further candidates —, failed fetches, Ed25519, and the chain workload."""
    names, pairs, cs = I.corpus()
    scans = SM.scan([p[0] for p in pairs], [p[1] for p in pairs], 64)
    wrong = [A.PublicKey(cases.K("rsa2048_01").pkcs1_der), None, A.PublicKey(cases.ED()[1].pub, "ed25519"), A.PublicKey(cases.K("rsa1024_01").pkcs1_der)]
    emails, cands = [], []
    for j, (c, sc) in enumerate(zip(cs, scans)):
        nc = min(sc.n_candidates, 21)
        row = [wrong[(j + k) % len(wrong)] for k in range(max(nc - 1, 0))] + ([c.email.public_key] if nc else [])
        emails.append(c.email)
        cands.append(row)
    doms, raws, resolver, unsigned = I.chain_workload(n=256)
    cscans = SM.scan(raws, doms, 8)
    for d, r, sc in zip(doms, raws, cscans):
        emails.append(A.Email(d, r, A.PublicKey(b"")))
        cands.append([resolver.get((d, s.selector)) for s in sc.sigs if s.code == 0])
    return emails, cands


@pytest.mark.parametrize("mode", MODES)
def test_selection_from_records_equals_selection_from_keys(mode):
    """Candidates as records to select_keys_from_records, as model-decoded keys to select_keys: records (all 192 bytes), chosen and
    the delivered keys identical.  max_sig_rounds=32: the corpus has an e-mail with 21 same-domain signatures."""
    eng = z.Engine(max_sig_rounds=32)
    try:
        emails, cands = selection_batches()
        rec_rows = [[record_of(k, i + j) for j, k in enumerate(row)] for i, row in enumerate(cands)]
        for i in range(0, len(rec_rows), 7):                     # an undecodable record in place of a wrong key, here and there
            if len(rec_rows[i]) > 1:
                rec_rows[i][0] = UNDECODABLE[(i // 7) % len(UNDECODABLE)]
        exp_infos = [M.decode_all([r or b"" for r in row], mode) for row in rec_rows]
        key_rows = [[M.public_key(x) for x in row] for row in exp_infos]
        recs, chosen, infos = eng.select_keys_from_records(emails, rec_rows, mode)
        xrecs, xchosen = eng.select_keys(emails, key_rows)
        assert [int(v) for v in chosen] == [int(v) for v in xchosen]
        for i, (a, b) in enumerate(zip(recs, xrecs)):
            assert a.tobytes() == b.tobytes(), (i, int(a["status"]), int(a["detail"]), int(b["status"]), int(b["detail"]))
        for i, (g, x, row) in enumerate(zip(infos, exp_infos, rec_rows)):
            assert_keys_equal(g, x, [r or b"" for r in row], f"e-mail {i}")
        n_ok = sum(int(v) != A.SEL_NONE for v in chosen)
        assert n_ok > 250 and A.SEL_NONE in [int(v) for v in chosen] and max(int(v) & 0x7FFFFFFF for v in chosen if int(v) != A.SEL_NONE) >= 19
        # the chosen key's bytes are what the record's public_key_hash was computed over
        import hashlib
        for i, ch in enumerate(chosen):
            if int(ch) != A.SEL_NONE:
                assert bytes(recs[i]["public_key_hash"]) == hashlib.sha256(infos[i][int(ch) & 0x7FFFFFFF].key).digest(), i
        # an undecodable record in front of a passing one moves the index by one and changes nothing else
        sub = [i for i, v in enumerate(chosen) if int(v) == 0][:40]
        assert len(sub) == 40
        shifted = [[UNDECODABLE[k % len(UNDECODABLE)]] + rec_rows[i] for k, i in enumerate(sub)]
        r2, c2, i2 = eng.select_keys_from_records([emails[i] for i in sub], shifted, mode)
        assert [int(v) for v in c2] == [1] * 40
        for k, i in enumerate(sub):
            assert r2[k].tobytes() == recs[i].tobytes() and i2[k][0].code != 0 and i2[k][1] == infos[i][0]
        # nothing to select from, cand_off that goes down, a key buffer one byte short
        r0, c0, i0 = eng.select_keys_from_records(emails[:3], [[], [], []], mode)
        assert [int(v) for v in c0] == [A.SEL_NONE] * 3 and i0 == [[], [], []] and all(int(s) == A.ZKE_DKIM_NOT_PASS for s in r0["status"])
        refs = A.EmailRefs(emails[:2])
        rows = [rec_rows[i] for i in sub[:2]]
        b = _KeyrecBuffers([r for row in rows for r in row])
        out, ch = np.zeros(2, A.RESULT_DTYPE), np.zeros(2, np.uint32)
        down = np.array([2, 1, 3], np.uint32)
        assert eng.lib.zke_select_keys_from_records(eng.h, refs.arr, 2, down.ctypes.data, b.arr, mode, out.ctypes.data, ch.ctypes.data, C.byref(b.c)) == E_ARG
        off = np.array([0, len(rows[0]), len(rows[0]) + len(rows[1])], np.uint32)
        refs = A.EmailRefs([emails[i] for i in sub[:2]])
        need = sum(len(x.key) for i in sub[:2] for x in exp_infos[i])
        b = _KeyrecBuffers([r for row in rows for r in row], need - 1)
        assert eng.lib.zke_select_keys_from_records(eng.h, refs.arr, 2, off.ctypes.data, b.arr, mode, out.ctypes.data, ch.ctypes.data, C.byref(b.c)) == E_NOMEM
        assert int(b.c.keys_need) == need and [int(v) for v in ch] == [0, 0] and out[0].tobytes() == recs[sub[0]].tobytes()     # the selection itself is delivered
        b = _KeyrecBuffers([r for row in rows for r in row], need)
        assert eng.lib.zke_select_keys_from_records(eng.h, refs.arr, 2, off.ctypes.data, b.arr, mode, out.ctypes.data, ch.ctypes.data, C.byref(b.c)) == 0
        b.c.infos_cap = int(off[2]) - 1
        assert eng.lib.zke_select_keys_from_records(eng.h, refs.arr, 2, off.ctypes.data, b.arr, mode, out.ctypes.data, ch.ctypes.data, C.byref(b.c)) == E_NOMEM
        assert int(b.c.infos_need) == int(off[2])
    finally:
        eng.close()


@pytest.mark.parametrize("mode", MODES)
def test_rfc8463_end_to_end_from_published_records(engine, mode):
    """The published message, its two selectors answered with the two published records: generate_email_inputs_from_records gives
    an Email that verifies — with both records, and for each signature when the other's record is withheld."""
    import test_rfc8463_vector as V
    r = K.rfc8463()
    answers = {(V.DOMAIN, r["ed25519"]["selector"].encode()): b"v=DKIM1; k=ed25519; p=" + r["ed25519"]["p_base64"].encode(),
               (V.DOMAIN, r["rsa"]["selector"].encode()): b"v=DKIM1; k=rsa; p=" + r["rsa"]["p_base64_spki"].encode()}
    asked = []

    def fetch(dom, sel):
        asked.append((dom, sel))
        return answers.get((dom, sel))
    ems = z.generate_email_inputs_from_records([V.DOMAIN], [V.RAW], fetch, mode=mode, engine=engine)
    assert sorted(asked) == sorted(answers) and ems[0].public_key == V.ED_KEY          # the Ed25519 signature is the first header
    assert int(engine.verify_emails(ems)[0]["status"]) == A.ZKE_OK
    for keep, want in ((r["ed25519"]["selector"].encode(), V.ED_KEY), (r["rsa"]["selector"].encode(), V.RSA_KEY)):
        ems = z.generate_email_inputs_from_records([V.DOMAIN], [V.RAW], lambda d, s: answers[(d, s)] if s == keep else None, mode=mode, engine=engine)
        assert ems[0].public_key == want and ems[0].raw_email == V.RAW
        rec = engine.verify_emails(ems)[0]
        assert (int(rec["status"]), int(rec["detail"])) == (A.ZKE_OK, 0)
    with pytest.raises(z.VerifyPanic) as ei:
        z.generate_email_inputs_from_records([V.DOMAIN], [V.RAW], lambda d, s: None, mode=mode, engine=engine)
    assert ei.value.reason == "No valid DKIM key found for any signature"
    with pytest.raises(z.VerifyPanic):            # a revoked key
        z.generate_email_inputs_from_records([V.DOMAIN], [V.RAW], lambda d, s: b"v=DKIM1; k=rsa; p=", mode=mode, engine=engine)


def test_generate_email_inputs_from_records_chain(engine):
    """The two-signature workload of the chain test with a resolver that answers TXT records: the same Email values as
    generate_email_inputs gives with the decoded keys."""
    doms, raws, resolver, unsigned = I.chain_workload(n=256)
    signed = [i for i in range(len(raws)) if i not in set(unsigned)]
    records = {k: record_of(v, j) for j, (k, v) in enumerate(sorted(resolver.items()))}
    a = z.generate_email_inputs_from_records([doms[i] for i in signed], [raws[i] for i in signed], lambda d, s: records.get((d, s)), engine=engine)
    b = z.generate_email_inputs([doms[i] for i in signed], [raws[i] for i in signed], lambda d, s: resolver.get((d, s)), engine=engine)
    assert a == b and len(a) == len(signed)
    assert (engine.verify_emails(a)["status"] == A.ZKE_OK).all()


def test_selections_from_records_beside_verify_batches_from_four_threads():
    """Selection from records on four slots beside ordinary verify batches from four host threads, synchronous and asynchronous
    forms mixed: every result identical to a serial run on the same engine."""
    eng = z.Engine(slots=4, host_threads=4)
    try:
        c3 = cases.multi_signature_case(3)
        cs = cases.build_cases()
        ok = [c for c in cs if c.status == A.ZKE_OK][:12]
        wrong = [A.PublicKey(cases.K("rsa2048_01").pkcs1_der), None, A.PublicKey(cases.ED()[0].pub, "ed25519")]
        sel_emails = [c3.email] * 4 + [c.email for c in ok]
        rows = [[record_of(wrong[k % 3], k), UNDECODABLE[k % len(UNDECODABLE)], record_of(c3.email.public_key, k)][k % 3:] for k in range(4)] + \
               [[record_of(wrong[k % 3], k), record_of(c.email.public_key, k)] for k, c in enumerate(ok)]
        dec = [r for _, r, _, _ in K.fixture_records()[::5]] + [c[2] for c in K.hand_cases()[::3]]
        wl = synth.make_workload("mt", 80, 2500, rsa_bits=2048, n_keys=4, seed=92, ragged=True, invalid_frac=0.1)
        serial = {"sel0": eng.select_keys_from_records(sel_emails, rows, M.ARCHIVE), "sel1": eng.select_keys_from_records(sel_emails, rows, M.DNS),
                  "dec": eng.decode_key_records(dec, M.DNS), "ver": eng.verify_emails(wl.emails)}
        assert sum(int(v) != A.SEL_NONE for v in serial["sel1"][1]) == len(sel_emails)
        errors = []

        def same_sel(got, exp):
            return got[0].tobytes() == exp[0].tobytes() and list(got[1]) == list(exp[1]) and got[2] == exp[2]

        def worker(t):
            try:
                for it in range(12):
                    kind = (t + it) % 4
                    if kind == 0:
                        assert same_sel(eng.select_keys_from_records(sel_emails, rows, M.ARCHIVE), serial["sel0"])
                    elif kind == 1:
                        ticket, r, ch, pend = eng.select_keys_from_records_async(sel_emails, rows, M.DNS)
                        r2 = eng.verify_emails(wl.emails)
                        eng.wait(ticket)
                        assert same_sel((r, ch, pend.result()), serial["sel1"]) and r2.tobytes() == serial["ver"].tobytes()
                    elif kind == 2:
                        ticket, pend = eng.decode_key_records_async(dec, M.DNS)
                        eng.wait(ticket)
                        assert pend.result() == serial["dec"]
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
        assert_keys_equal(serial["dec"], M.decode_all(dec, M.DNS), dec, "serial run")
    finally:
        eng.close()


def test_a_selection_nobody_waits_for_is_delivered():
    """The ticket protocol: a selection from records that is never waited for delivers when its slot is reused, and on destroy."""
    eng = z.Engine(slots=1)
    c = [c for c in cases.build_cases() if c.status == A.ZKE_OK][0]
    row = [[UNDECODABLE[0], record_of(c.email.public_key)]]
    t1, r1, ch1, p1 = eng.select_keys_from_records_async([c.email], row, M.DNS)
    eng.verify_emails([c.email])                              # the slot's next batch retires the selection
    assert int(ch1[0]) == 1 and int(r1[0]["status"]) == A.ZKE_OK and p1.result()[0][1].key == c.email.public_key.key
    t2, r2, ch2, p2 = eng.select_keys_from_records_async([c.email], row, M.ARCHIVE)
    eng.close()                                               # ... and so does destroy
    assert int(ch2[0]) == 1 and int(r2[0]["status"]) == A.ZKE_OK and p2.result()[0][1].key == c.email.public_key.key
