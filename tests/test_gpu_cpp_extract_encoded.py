"""GPU: Engine::extract_captures_encoded and Engine::utf8_lossy of the C++ mirror (include/zkemail_core.hpp,
tests/cpp/extract_encoded_test.cpp) on four signed e-mails whose subject and body carry ill-formed UTF-8, one of which fails its
signature: every line the program prints against values built here from the inputs alone — the strings Python's
decode("utf-8", "replace") gives for the bytes the patterns capture, zkemail_rs_amd.abi_encode.abi_encode over them, hashlib.sha256."""
import hashlib
import re
import subprocess

import numpy as np
import pytest

import synth
import utf8_lossy_cases as U
from zkemail_rs_amd import _abi as A
from zkemail_rs_amd import build
from zkemail_rs_amd import regex_compile as rc
from zkemail_rs_amd.abi_encode import abi_encode

pytestmark = pytest.mark.gpu

SUBJECT, BODY = r"subject:([^\r\n]+)\r\n", r"V<([^>]*)>"
CONTENT = [b"caf\xc3\xa9", U.UNICODE_EXAMPLE, b"\xff" * 40, b"\xf0\x9f\x98"]


def test_cpp_mirror_extracts_repairs_and_encodes(tmp_path):
    exe = build.build_cpp_extract_encoded()
    key = synth.keys_of(1024, 1)[0]
    args, subjects = [], []
    for i, c in enumerate(CONTENT):
        subject = b"re \xc0 %d" % i
        hs = [(n, subject if n == b"Subject" else v) for n, v in synth.std_headers(np.random.default_rng(40 + i), i, "example.com")]
        raw, _ = synth.sign_email(hs, b"first\r\nV<" + c + b">\r\nlast\r\n", key, synth.SignSpec(domain="example.com"), corrupt="body" if i == 2 else None)
        (tmp_path / f"m{i}.eml").write_bytes(raw)
        (tmp_path / f"m{i}.key").write_bytes(key.pkcs1_der)
        args.append(str(tmp_path / f"m{i}"))
        subjects.append(subject)
    for name, pat in (("h0", SUBJECT), ("b0", BODY)):
        dfa = rc.create_dfa(pat, unicode=False)
        for ext, data in (("fwd", dfa.fwd), ("bwd", dfa.bwd), ("prog", rc.create_capture_program(pat, unicode=False))):
            (tmp_path / f"{name}.{ext}").write_bytes(data)
    r = subprocess.run([exe, str(tmp_path / "h0"), str(tmp_path / "b0"), "--"] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.splitlines()
    enc = [ln.split(" ") for ln in lines if ln.startswith("enc ")]
    strs = [ln.split(" ") for ln in lines if ln.startswith("str ")]
    assert len(enc) == len(strs) == len(CONTENT)
    for i, c in enumerate(CONTENT):
        if i == 2:                               # the signature does not verify: no strings, no bytes, a zero digest
            assert int(enc[i][2]) != A.ZKE_OK and enc[i][4] == "00" * 32 and enc[i][5] == "" and strs[i] == ["str", "2"]
            continue
        want = [U.reference(subjects[i]), U.reference(b"V<" + c + b">"), U.reference(c)]
        assert [bytes.fromhex(x[1:]) for x in strs[i][2:]] == want, i
        out = A.EmailVerifierOutput(hashlib.sha256(b"example.com").digest(), hashlib.sha256(key.pkcs1_der).digest(),
                                    ["name%d" % i, "value%d" % i] if i % 2 == 0 else [])
        ref = abi_encode(out, [w.decode() for w in want])
        assert [int(enc[i][1]), int(enc[i][2]), int(enc[i][3])] == [i, A.ZKE_OK, 1]
        assert enc[i][5] == ref.hex() and enc[i][4] == hashlib.sha256(ref).hexdigest(), i
    assert "same 1" in lines
    assert [ln for ln in lines if ln.startswith("lossy ")] == ["lossy " + U.pins()[0][1].hex() + " 1 0"]
    assert not re.search(r"^ERROR", r.stdout, flags=re.M)
