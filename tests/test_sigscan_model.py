"""CPU (-m "not gpu"): the scan and selection models of tests/sigscan_model.py — the expected values of tests/test_gpu_sigscan.py —
against what is known without them: the corpus' own expectations, the tag-list fuzz generator's verdicts, the strictness cases
derived in tests/strict_cases.py, the signer's own selector and domain.  And the new C-ABI surface that needs no GPU: the struct
layouts of the ctypes mirrors against the header (through a C compiler), and the refusal of null arguments."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from zkemail_rs_amd import _abi as A
from zkemail_rs_amd import engine

import cases
import sigscan_inputs as I
import sigscan_model as M
import strict_cases as S
import synth
from synth import SignSpec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_model_over_the_corpus():
    names, pairs, cs = I.corpus()
    scans = M.scan([p[0] for p in pairs], [p[1] for p in pairs], max_sigs=A.SCAN_MAX_SIGS)
    codes = {}
    for nm, c, sc in zip(names, cs, scans):
        if c.status == A.ZKE_OK:
            assert sc.status == A.ZKE_OK and sc.n_candidates >= 1, nm
        if c.status == A.ZKE_PARSE_FAIL:
            assert (sc.status, sc.detail) == (A.ZKE_PARSE_FAIL, c.detail if c.detail is not None else sc.detail) and not sc.sigs, nm
        if c.status == A.ZKE_UNSUPPORTED and c.detail in (A.D_U_TOO_MANY_HEADERS, A.D_U_DOMAIN_FOLD, A.D_U_MIME_CTYPE, A.D_U_MIME_BOUNDARY, A.D_U_MIME_DEPTH):
            assert (sc.status, sc.detail) == (A.ZKE_UNSUPPORTED, c.detail), nm
        if c.status == A.ZKE_DKIM_NOT_PASS and c.detail in (A.D_SIG_SYNTAX, A.D_MISSING_TAG, A.D_INCOMPATIBLE_VERSION, A.D_DOMAIN_MISMATCH,
                                                             A.D_FROM_NOT_SIGNED, A.D_BAD_QUERY_METHOD):
            assert c.detail in [s.code for s in sc.sigs], nm          # validate_header's refusal is the verify path's detail
        assert sc.n_signatures == len(sc.sigs) and sc.n_candidates == sum(s.code == 0 for s in sc.sigs), nm
        for s in sc.sigs:
            codes[s.code] = codes.get(s.code, 0) + 1
    # every code the scan can report is met by these inputs
    for code in (0, A.D_NEUTRAL, A.D_FROM_NOT_SIGNED, A.D_DOMAIN_MISMATCH, A.D_BAD_QUERY_METHOD, A.D_INCOMPATIBLE_VERSION, A.D_MISSING_TAG,
                 A.D_SIG_SYNTAX, A.D_U_SIG_NON_ASCII, A.D_U_TOO_MANY_TAGS, A.D_U_SIG_TOO_LONG):
        assert codes.get(code), (code, codes)
    assert codes[0] > 100 and max(sc.n_signatures for sc in scans) == 21


def test_model_over_the_taglist_fuzz_headers():
    pairs, kinds, emails = I.taglist_headers()
    assert len(pairs) == 4096
    n_ok = 0
    for (raw, dom), kind, em in zip(pairs, kinds, emails):
        sc = M.scan_email(raw, dom)
        if sc.status != A.ZKE_OK:          # a byte the generator broke on purpose may break parse_mail itself
            assert kind == "broken" and not sc.sigs, raw[:400]
            continue
        assert sc.n_signatures == 1, raw[:400]
        s = sc.sigs[0]
        assert raw[s.value_span[0]:s.value_span[1]] and raw[:s.value_span[0]].rstrip(b" ").endswith(b"DKIM-Signature:")
        if kind == "ok":          # the generator's knowledge: signed for example.com under sel1 with the key's algorithm
            n_ok += 1
            want = A.SIG_ALGO_ED25519_SHA256 if em.public_key.key_type == "ed25519" else A.SIG_ALGO_RSA_SHA256
            assert (s.code, s.selector, s.algo) == (0, b"sel1", want), raw[:600]
    assert n_ok > 2500


@pytest.mark.parametrize("flagged", [False, True])
def test_model_on_the_strictness_cases(flagged):
    for case in S.plain_cases():
        name, flag, em, d0, d1 = case[:5]
        st, det = d1 if flagged else d0
        strict = A.strict_mask(**{flag: 1}) if flagged else 0
        sc = M.scan_email(em.raw_email, em.from_domain, strict=strict, now=S.NOW)
        assert sc.status == A.ZKE_OK and sc.n_signatures == 1, name
        code = sc.sigs[0].code
        if flag == "b_removes_own_span_only" or st == A.ZKE_OK:
            assert code == 0, (name, flagged, code)          # b= handling is no part of validate_header
        else:
            assert code == det, (name, flagged, code, det)


def test_model_against_the_signers_knowledge():
    rng = np.random.default_rng(3)
    k0, ed = cases.K("rsa2048_00"), cases.ED()[0]
    for i in range(200):
        dom = ["example.com", "Mail.Example.ORG", "a.b.c.example.net"][i % 3]
        sel = "".join("abcdefghijklmnopqrstuvwxyz0123456789._-"[int(x)] for x in rng.integers(0, 39, int(rng.integers(1, 40))))
        algo = ["rsa-sha256", "rsa-sha1"][i % 2]
        key = ed if i % 7 == 0 else k0
        spec = SignSpec(domain=dom, selector=sel, algo="rsa-sha256" if key is ed else algo, header_canon=["relaxed", "simple"][i % 2])
        raw, _ = synth.sign_email(synth.std_headers(rng, i, "example.com"), synth.ascii_body(rng, 80), key, spec)
        frm = dom.upper() if i % 5 == 0 else (dom if i % 11 else "elsewhere.org")
        sc = M.scan_email(raw, frm)
        assert sc.status == A.ZKE_OK and len(sc.sigs) == 1
        s = sc.sigs[0]
        assert s.selector == sel.encode() and s.code == (0 if frm.lower() == dom.lower() else A.D_NEUTRAL)
        assert s.algo == (A.SIG_ALGO_ED25519_SHA256 if key is ed else [A.SIG_ALGO_RSA_SHA256, A.SIG_ALGO_RSA_SHA1][i % 2])
        assert s.header_index == 0 and raw[s.value_span[0]:s.value_span[0] + 4] == b"v=1;"


def test_model_lists_the_first_max_sigs_and_counts_all():
    raw, dom = I.email_with_signatures(21)
    full = M.scan_email(raw, dom, max_sigs=64)
    assert full.n_signatures == 21 and len(full.sigs) == 21 and {s.code for s in full.sigs} == {0, A.D_NEUTRAL, A.D_FROM_NOT_SIGNED, A.D_INCOMPATIBLE_VERSION}
    for ms in (1, 8, 20, 21):
        cut = M.scan_email(raw, dom, max_sigs=ms)
        assert cut.sigs == full.sigs[:ms] and (cut.n_signatures, cut.n_candidates) == (21, full.n_candidates)
    pairs, sels = I.selector_emails()
    for (r, d), sel in zip(pairs, sels):
        sc = M.scan_email(r, d)
        assert [s.selector for s in sc.sigs] == [sel] and sc.sigs[0].code == 0, len(sel)


def test_selection_model_on_a_multi_signature_email():
    """multi_signature_case(3) under [a wrong RSA key, a failed fetch, an Ed25519 key, the right key, the right key]: the third is
    outside what the engine implements, the fourth is chosen and says so in bit 31."""
    c = cases.multi_signature_case(3)
    right = c.email.public_key
    keys = [A.PublicKey(cases.K("rsa2048_01").pkcs1_der), None, A.PublicKey(cases.ED()[0].pub, "ed25519"), right, right]
    recs, chosen = M.select_keys([c.email], [keys])
    assert int(chosen[0]) == 3 | A.SEL_AFTER_UNSUPPORTED and int(recs[0]["status"]) == A.ZKE_OK
    recs, chosen = M.select_keys([c.email, c.email, c.email], [keys[:3], [], [right]])
    assert [int(x) for x in chosen] == [A.SEL_NONE, A.SEL_NONE, 0]
    assert (int(recs[0]["status"]), int(recs[0]["detail"])) == (A.ZKE_UNSUPPORTED, A.D_U_ALGO_ED25519)
    assert (int(recs[1]["status"]), int(recs[1]["detail"])) == (A.ZKE_DKIM_NOT_PASS, A.D_NEUTRAL)


def test_new_struct_layouts_match_the_header(tmp_path):
    """sizeof / offsetof as a C compiler reads include/zkemail_amd.h, against the ctypes mirrors field by field."""
    structs = {"zke_sig_info": A.zke_sig_info, "zke_sig_scan": A.zke_sig_scan, "zke_key_ref": A.zke_key_ref}
    lines = []
    for sname, cls in structs.items():
        lines.append(f'printf("{sname} %zu\\n", sizeof({sname}));')
        for f, _ in cls._fields_:
            lines.append(f'printf("{sname}.{f} %zu\\n", offsetof({sname}, {f}));')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zkemail_amd.h"\nint main(void) {\n' + "\n".join(lines) +
                   '\nprintf("consts %u %u %u\\n", ZKE_SCAN_MAX_SIGS, ZKE_SEL_NONE, ZKE_SEL_AFTER_UNSUPPORTED);\nreturn 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines() if not l.startswith("consts"))
    for sname, cls in structs.items():
        assert int(got[sname]) == C.sizeof(cls), sname
        for f, _ in cls._fields_:
            assert int(got[f"{sname}.{f}"]) == getattr(cls, f).offset, (sname, f)
    assert C.sizeof(A.zke_sig_info) == 32 and A.SIG_INFO_DTYPE.itemsize == 32 and C.sizeof(A.zke_key_ref) == 24
    assert [n for n in A.SIG_INFO_DTYPE.names] == [f for f, _ in A.zke_sig_info._fields_]
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    assert f"consts {A.SCAN_MAX_SIGS} {A.SEL_NONE} {A.SEL_AFTER_UNSUPPORTED}" in out
    assert C.sizeof(A.zke_options) == 104 and C.sizeof(A.zke_result) == 192          # untouched by the additions


def test_null_arguments_are_refused():
    lib = engine.load_library()
    E_ARG = -1
    t = C.c_uint64()
    scan = A.zke_sig_scan()
    refs = A.EmailRefs([A.Email("example.com", b"From: a@example.com\r\n\r\nx\r\n", A.PublicKey(b""))])
    out = np.zeros(1, A.RESULT_DTYPE)
    chosen = np.zeros(1, np.uint32)
    off = np.zeros(2, np.uint32)
    keys = (A.zke_key_ref * 1)()
    assert lib.zke_scan_signatures(None, refs.arr, 1, 8, C.byref(scan)) == E_ARG
    assert lib.zke_scan_signatures(None, None, 0, 8, None) == E_ARG
    assert lib.zke_scan_signatures_async(None, refs.arr, 1, 8, C.byref(scan), C.byref(t)) == E_ARG
    assert lib.zke_scan_signatures_async(None, refs.arr, 1, 8, C.byref(scan), None) == E_ARG
    assert lib.zke_select_keys(None, refs.arr, 1, off.ctypes.data, keys, out.ctypes.data, chosen.ctypes.data) == E_ARG
    assert lib.zke_select_keys(None, None, 0, None, None, None, None) == E_ARG
    assert lib.zke_select_keys_async(None, refs.arr, 1, off.ctypes.data, keys, out.ctypes.data, chosen.ctypes.data, C.byref(t)) == E_ARG
    assert lib.zke_select_keys_async(None, refs.arr, 1, off.ctypes.data, keys, out.ctypes.data, chosen.ctypes.data, None) == E_ARG
    assert {"zke_scan_signatures", "zke_scan_signatures_async", "zke_select_keys", "zke_select_keys_async"} <= set(engine.EXPORTED_SYMBOLS)
