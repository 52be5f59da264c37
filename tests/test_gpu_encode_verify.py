"""GPU: zke_verify_emails_encoded, synchronous and asynchronous, over 48 signed e-mails (tests/synth.py, the 1 024-bit keys of
tests/golden/keys.json, external inputs on every second e-mail) in the three forms of zke_encode_in:

    plain   both lists NULL: zke_verify_emails' pipeline, kind 0 for every e-mail
    lists   one part list, 1 header part + 1 body part, under both DFA mappings: kind 1
    mixed   two configs (a header part; a header part and a body part) plus ZKE_CONFIG_NONE: kinds 1, 1 and 0

Conditions, asserted: the records equal the plain entry's (zke_verify_emails / _with_regex / _mixed) on the same batch byte for byte;
the batch is built so that exactly four NAMED e-mails can fail — a tampered body (ZKE_DKIM_NOT_PASS), a null external input
(ZKE_EXTERNAL_INPUT_NULL), a header part whose capture its match does not hold (ZKE_HEADER_REGEX_FAIL), a body part likewise
(ZKE_BODY_REGEX_FAIL) — and every other e-mail is ZKE_OK and encoded.  (verify_email reads no regex part: in the plain form the two
regex e-mails pass like the rest, and in the mixed form each of the four sits under a config that can show its failure.)  Every
encoding and digest against zkemail_rs_amd.abi_encode.abi_encode and hashlib.sha256, built from the inputs alone (the two witness
hashes are SHA-256 of from_domain and of the key bytes, circuits.rs:16-17).  And the exact-size protocol: infos_cap or bytes_cap one
short fails at once with ZKE_E_NOMEM.  One engine per case with ONE slot: sync and async runs share its output buffer."""
import copy
import hashlib

import numpy as np
import pytest

import synth
import zkemail_rs_amd as z
from zkemail_rs_amd import _abi as A
from zkemail_rs_amd.abi_encode import abi_encode
from zkemail_rs_amd.engine import regex_matches_of

pytestmark = pytest.mark.gpu

N = 48
TAMPERED, NULL_EXT, HDR_FAIL, BODY_FAIL = 5, 17, 30, 40          # (mod 3: none, none, config 0, config 1 in the mixed form)
ZERO = b"\0" * 32


def _batch():
    """48 passing EmailWithRegex inputs with one header part and one body part, then the four named e-mails spoilt."""
    inputs, _, expect = synth.make_regex_workload("encoded", N, 600, rsa_bits=1024, n_keys=2, seed=61, n_header_parts=1, n_body_parts=1)
    assert not any(expect)
    for i, inp in enumerate(inputs):
        if i % 2 == 0:
            inp.email.external_inputs = [A.ExternalInput("address", "0x%040x" % (i * 7919)), A.ExternalInput("näme%d" % i, "välue €" * (i % 5))][:1 + i % 2 + (i % 4 == 0)]
    raw = inputs[TAMPERED].email.raw_email
    inputs[TAMPERED].email.raw_email = raw[:-9] + bytes([raw[-9] ^ 1]) + raw[-8:]
    inputs[NULL_EXT].email.external_inputs = [A.ExternalInput("present", "x"), A.ExternalInput("absent", None)]
    inputs[HDR_FAIL].regex_info.header_parts[0].captures = ["nobody-wrote-this"]
    inputs[BODY_FAIL].regex_info.body_parts[0].captures = ["nobody-wrote-this"]
    return inputs


def _form_inputs(form):
    inputs = _batch()
    if form == "plain":
        return [i.email for i in inputs]
    if form == "mixed":
        out = []
        for k, i in enumerate(inputs):
            out.append(A.EmailWithRegex(i.email, A.RegexInfo(i.regex_info.header_parts, None)) if k % 3 == 0 else i if k % 3 == 1 else i.email)
        return out
    return inputs


def _named(form):
    st = {TAMPERED: A.ZKE_DKIM_NOT_PASS, NULL_EXT: A.ZKE_EXTERNAL_INPUT_NULL, HDR_FAIL: A.ZKE_HEADER_REGEX_FAIL, BODY_FAIL: A.ZKE_BODY_REGEX_FAIL}
    if form == "plain":
        st[HDR_FAIL] = st[BODY_FAIL] = A.ZKE_OK
    return st


def _plain_entry(eng, form, inputs):
    return eng.verify_emails(inputs) if form == "plain" else eng.verify_emails_with_regex(inputs) if form == "lists" else eng.verify_emails_mixed(inputs)


def _check(form, inputs, records, encoded, infos, plain):
    assert records.tobytes() == plain.tobytes(), "records differ from the plain entry's"
    named = _named(form)
    off = 0
    for i, inp in enumerate(inputs):
        em = inp if isinstance(inp, A.Email) else inp.email
        want_status = named.get(i, A.ZKE_OK)
        assert int(records[i]["status"]) == want_status, (form, i, int(records[i]["status"]), int(records[i]["detail"]))
        out = A.EmailVerifierOutput(hashlib.sha256(em.from_domain.encode()).digest(), hashlib.sha256(em.public_key.key).digest(),
                                    A.flat_external_inputs(em.external_inputs))
        ref = abi_encode(out) if isinstance(inp, A.Email) else abi_encode(out, regex_matches_of(inp))
        kind = A.ENC_KIND_EMAIL if isinstance(inp, A.Email) else A.ENC_KIND_WITH_REGEX
        assert (int(infos[i]["off"]), int(infos[i]["kind"])) == (off, kind), (form, i)
        if want_status == A.ZKE_OK:
            assert int(infos[i]["len"]) == len(ref) and encoded[i] == (ref, hashlib.sha256(ref).digest()), (form, i)
        else:
            assert int(infos[i]["len"]) == 0 and encoded[i] == (b"", ZERO), (form, i)
        off += len(ref)
    assert sum(1 for e, _ in encoded if e) == N - sum(1 for s in named.values() if s != A.ZKE_OK)


CASES = [("plain", 0), ("lists", 1), ("lists", 2), ("mixed", 0)]


@pytest.mark.parametrize("form,mapping", CASES, ids=[f"{f}-dfa{m}" for f, m in CASES])
def test_verify_emails_encoded_sync_and_async(form, mapping):
    eng = z.Engine(slots=1, dfa_mapping=mapping)
    try:
        inputs = _form_inputs(form)
        plain = _plain_entry(eng, form, copy.deepcopy(inputs))
        assert sum(1 for r in plain if r["status"] != A.ZKE_OK) == (2 if form == "plain" else 4)
        c = _sync_call(eng, inputs, form)
        _check(form, inputs, c.records, c.enc.result(), c.enc.infos, plain)
        records, encoded = eng.verify_emails_encoded(inputs, form=form)
        assert records.tobytes() == plain.tobytes() and encoded == c.enc.result()
        ticket, pending = eng.verify_emails_encoded_async(inputs, form=form)
        eng.wait(ticket)
        _check(form, inputs, pending.records, pending.enc.result(), pending.enc.infos, plain)
        assert (pending.enc.c.infos_need, pending.enc.c.bytes_need) == (N, sum(c.planned))
        # the too-small-buffer protocol: both sizes are exact and known before anything is staged
        for kw in (dict(infos_cap=N - 1), dict(bytes_cap=sum(c.planned) - 1)):
            with pytest.raises(z.EngineError, match=r"\(-3\)"):
                eng.verify_emails_encoded(inputs, form=form, **kw)
        records, encoded = eng.verify_emails_encoded(inputs, form=form, bytes_cap=sum(c.planned) + 1)
        assert records.tobytes() == plain.tobytes() and [e for e, _ in encoded] == [e for e, _ in pending.enc.result()]
    finally:
        eng.close()


def _sync_call(eng, inputs, form):
    """The synchronous entry with its call object in hand (Engine.verify_emails_encoded returns the readings, not the info array)."""
    import ctypes as C
    c = eng._encoded_call(inputs, form, None, None)
    eng._check(eng.lib.zke_verify_emails_encoded(eng.h, c.refs.arr, c.refs.n, C.byref(c.c), c.out.ctypes.data, C.byref(c.enc.c)), "zke_verify_emails_encoded")
    return c
