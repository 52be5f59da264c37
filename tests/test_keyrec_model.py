"""CPU (-m "not gpu"): the key-record model of tests/keyrec_model.py — the expected values of tests/test_gpu_keyrec.py — against
what is known without it: openssl's own SubjectPublicKeyInfo encoding of every fixture key, the two records RFC 8463 A.2 publishes
and the keys tests/test_rfc8463_vector.py verifies the message under, and hand-written cases with the code each rule gives.  And
the new C-ABI surface that needs no GPU: struct layouts against the header through a C compiler, the refusal of null arguments."""
import base64
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from zkemail_rs_amd import _abi as A
from zkemail_rs_amd import engine

import keyrec_cases as K
import keyrec_model as M
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (M.ARCHIVE, M.DNS)


@pytest.mark.skipif(shutil.which("openssl") is None, reason="openssl is not installed")
def test_every_fixture_key_through_openssl(tmp_path):
    """pkcs1_der -> openssl's SubjectPublicKeyInfo -> p=base64 -> the model returns pkcs1_der again; likewise p=base64(pkcs1_der)."""
    for name, k in sorted(synth.load_keys().items()):
        src = tmp_path / (name + ".der")
        src.write_bytes(k.pkcs1_der)
        spki = subprocess.run(["openssl", "rsa", "-RSAPublicKey_in", "-inform", "DER", "-in", str(src), "-pubout", "-outform", "DER"],
                              check=True, capture_output=True).stdout
        assert spki == K.spki_wrap(k.pkcs1_der), name                     # the tests' own wrapper is openssl's encoding
        assert spki.endswith(k.pkcs1_der), name                           # "re-encode" is "take the slice"
        for mode in MODES:
            for der in (spki, k.pkcs1_der):
                got = M.decode(b"v=DKIM1; k=rsa; p=" + base64.b64encode(der), mode)
                assert got == M.Key(0, A.KEY_RSA, k.pkcs1_der), (name, mode)


def test_fixture_records_decode_in_both_modes():
    recs = K.fixture_records()
    assert len(recs) == 2 * len(synth.load_keys()) + 4 + 2
    for name, rec, kt, key in recs:
        for mode in MODES:
            got = M.decode(rec, mode)
            assert (got.code, got.key_type) == (0, kt), (name, mode, got.code)
            if key is not None:
                assert got.key == key, (name, mode)


def test_rfc8463_records_give_the_keys_the_vector_verifies_under():
    """The two records RFC 8463 A.2 publishes decode to test_rfc8463_vector.RSA_KEY / ED_KEY, the keys under which that file's
    tests verify the published message (its RSA key is the JSON's pkcs1_der_hex, transcribed independently of p_base64_spki)."""
    import test_rfc8463_vector as V
    r = K.rfc8463()
    for mode in MODES:
        rsa = M.decode(b"v=DKIM1; k=rsa; p=" + r["rsa"]["p_base64_spki"].encode(), mode)
        ed = M.decode(b"v=DKIM1; k=ed25519; p=" + r["ed25519"]["p_base64"].encode(), mode)
        assert rsa == M.Key(0, A.KEY_RSA, V.RSA_KEY.key), mode
        assert ed == M.Key(0, A.KEY_ED25519, V.ED_KEY.key), mode
        assert M.public_key(rsa) == V.RSA_KEY and M.public_key(ed) == V.ED_KEY


@pytest.mark.parametrize("case", K.hand_cases(), ids=lambda c: f"{'archive' if c[1] == 0 else 'dns'}: {c[0]}")
def test_hand_written_cases(case):
    name, mode, rec, code, kt, key = case
    got = M.decode(rec, mode)
    assert (got.code, got.key_type, got.key) == (code, kt, key), (name, A.KEYREC_NAMES.get(got.code), A.KEYREC_NAMES.get(code))


def test_every_code_is_met_by_the_hand_written_cases():
    codes = {(c[1], c[3]) for c in K.hand_cases()}
    for code in (0, A.D_KEYREC_NO_KEY, A.D_KEYREC_B64, A.D_KEYREC_TYPE, A.D_KEYREC_DER, A.D_KEYREC_RANGE, A.D_KEYREC_ED25519_LEN):
        assert (M.ARCHIVE, code) in codes and (M.DNS, code) in codes or code in (A.D_KEYREC_DER,), code
    assert (M.ARCHIVE, A.D_KEYREC_NON_ASCII_EDGE) in codes and (M.DNS, A.D_KEYREC_VERSION) in codes and (M.DNS, A.D_KEYREC_SYNTAX) in codes


def test_limits():
    for mode in MODES:
        for rec, code, key in K.limit_records(mode):
            got = M.decode(rec, mode)
            assert (got.code, got.key) == (code, key), (mode, len(rec))
    assert [len(r) for r, _, _ in K.limit_records(0)] == [4095, 4096, 4097]


def test_strict_base64():
    assert M.b64_standard(b"AAAA") == b"\0\0\0" and M.b64_standard(b"AA==") == b"\0" and M.b64_standard(b"AAA=") == b"\0\0"
    for bad in (b"AAA", b"AA", b"A", b"AB==", b"AAB=", b"A===", b"====", b"AA=A", b"AA A", b"AAAA\n", b"AA-_", b"=AAA"):
        assert M.b64_standard(bad) is None, bad
    rng = np.random.default_rng(5)
    for n in range(0, 70):
        raw = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert M.b64_standard(base64.b64encode(raw)) == raw


@pytest.mark.parametrize("mode", MODES)
def test_mutation_fuzz_shares(mode):
    """The 4 096 seeded records of the GPU fuzz, against the model alone: at least a quarter decode, at least a quarter fail, and
    no record is outside what the model answers (mutation bytes are printable ASCII, tab, CR, LF: no non-ASCII edge)."""
    recs = K.fuzz_records(seed=100 + mode)
    assert len(recs) == 4096
    keys = M.decode_all(recs, mode)
    ok = sum(k.code == 0 for k in keys)
    assert ok >= 1024 and len(keys) - ok >= 1024, (ok, len(keys))
    assert not any(k.code in (A.D_KEYREC_NON_ASCII_EDGE, A.D_KEYREC_TOO_LONG) for k in keys)
    assert all(b < 0x80 for r in recs for b in r)
    # a decoded RSA key is a slice of what p= decodes to; an Ed25519 key is 32 bytes
    for r, k in zip(recs, keys):
        if k.code == 0:
            assert len(k.key) == 32 if k.key_type == A.KEY_ED25519 else (k.key[:1] == b"\x30" and M.pkcs1(k.key) == 0)


def test_new_struct_layouts_match_the_header(tmp_path):
    """sizeof / offsetof as a C compiler reads include/zkemail_amd.h, against the ctypes mirrors field by field."""
    structs = {"zke_keyrec_ref": A.zke_keyrec_ref, "zke_key_info": A.zke_key_info, "zke_keyrec_out": A.zke_keyrec_out}
    lines = []
    for sname, cls in structs.items():
        lines.append(f'printf("{sname} %zu\\n", sizeof({sname}));')
        for f, _ in cls._fields_:
            lines.append(f'printf("{sname}.{f} %zu\\n", offsetof({sname}, {f}));')
    consts = ["ZKE_KEYREC_ARCHIVE", "ZKE_KEYREC_DNS", "ZKE_KEYREC_MAX_BYTES"] + \
             ["ZKE_D_KEYREC_" + n for n in ("NO_KEY", "B64", "TYPE", "DER", "RANGE", "ED25519_LEN", "VERSION", "SYNTAX", "NON_ASCII_EDGE", "TOO_LONG")]
    lines += [f'printf("{c} %u\\n", (unsigned){c});' for c in consts]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zkemail_amd.h"\nint main(void) {\n' + "\n".join(lines) + '\nreturn 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for sname, cls in structs.items():
        assert int(got[sname]) == C.sizeof(cls), sname
        for f, _ in cls._fields_:
            assert int(got[f"{sname}.{f}"]) == getattr(cls, f).offset, (sname, f)
    assert C.sizeof(A.zke_key_info) == 16 == A.KEY_INFO_DTYPE.itemsize and C.sizeof(A.zke_keyrec_ref) == 16 and C.sizeof(A.zke_keyrec_out) == 48
    assert [n for n in A.KEY_INFO_DTYPE.names] == [f for f, _ in A.zke_key_info._fields_]
    for c in consts:
        py = c[4:] if c.startswith("ZKE_D_") else c[4:]
        assert int(got[c]) == getattr(A, py), c
    assert C.sizeof(A.zke_options) == 104 and C.sizeof(A.zke_result) == 192          # untouched by the additions


def test_null_arguments_are_refused():
    lib = engine.load_library()
    E_ARG = -1
    t = C.c_uint64()
    out = A.zke_keyrec_out()
    recs = (A.zke_keyrec_ref * 1)()
    refs = A.EmailRefs([A.Email("example.com", b"From: a@example.com\r\n\r\nx\r\n", A.PublicKey(b""))])
    res = np.zeros(1, A.RESULT_DTYPE)
    chosen = np.zeros(1, np.uint32)
    off = np.zeros(2, np.uint32)
    assert lib.zke_decode_key_records(None, recs, 1, 0, C.byref(out)) == E_ARG
    assert lib.zke_decode_key_records(None, None, 0, 0, None) == E_ARG
    assert lib.zke_decode_key_records_async(None, recs, 1, 1, C.byref(out), C.byref(t)) == E_ARG
    assert lib.zke_select_keys_from_records(None, refs.arr, 1, off.ctypes.data, recs, 1, res.ctypes.data, chosen.ctypes.data, C.byref(out)) == E_ARG
    assert lib.zke_select_keys_from_records_async(None, None, 0, None, None, 0, None, None, None, None) == E_ARG
    assert {"zke_decode_key_records", "zke_decode_key_records_async", "zke_select_keys_from_records",
            "zke_select_keys_from_records_async"} <= set(engine.EXPORTED_SYMBOLS)
