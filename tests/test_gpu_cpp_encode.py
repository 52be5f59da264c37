"""GPU: the encoded batch calls of the C++ mirror (include/zkemail_core.hpp, tests/cpp/encode_test.cpp) — verify_emails_encoded
and verify_emails_with_regex_encoded over eight signed e-mails with one header part and one body part, external inputs on some of
them, one with a null value and one with a capture its match does not hold.  Every line the program prints against
zkemail_rs_amd.abi_encode.abi_encode and hashlib.sha256, built from the inputs alone."""
import hashlib
import os
import subprocess
import tempfile

import pytest

import synth
from zkemail_rs_amd import _abi as A
from zkemail_rs_amd import build
from zkemail_rs_amd.abi_encode import abi_encode
from zkemail_rs_amd.engine import regex_matches_of

pytestmark = pytest.mark.gpu

N = 8


def ext_of(i):
    """What tests/cpp/encode_test.cpp gives e-mail i (the flattened list; None: a null value)."""
    x = []
    if i % 2 == 0:
        x += ["name%d" % i, "value%d" % i]
    if i % 4 == 0:
        x += ["a", "", "", "b"]
    return None if i == 3 else x


def test_cpp_mirror_encodes_batches():
    exe = build.build_cpp_encode()
    inputs, _, _ = synth.make_regex_workload("cpp-encoded", N, 500, rsa_bits=1024, n_keys=2, seed=88, n_header_parts=1, n_body_parts=1)
    inputs[5].regex_info.body_parts[0].captures = ["nobody-wrote-this"]
    with tempfile.TemporaryDirectory() as tmp:
        args = []
        for k, inp in enumerate(inputs):
            for ext, data in (("eml", inp.email.raw_email), ("key", inp.email.public_key.key)):
                with open(os.path.join(tmp, f"m{k}.{ext}"), "wb") as f:
                    f.write(data)
            args.append(os.path.join(tmp, f"m{k}"))
        pats = [tmp + "/h0.dfa", tmp + "/b0.dfa"]
        for path, part in zip(pats, (inputs[0].regex_info.header_parts[0], inputs[0].regex_info.body_parts[0])):
            open(path + ".fwd", "wb").write(part.verify_re.fwd)
            open(path + ".bwd", "wb").write(part.verify_re.bwd)
        caps = os.path.join(tmp, "caps.txt")
        with open(caps, "w") as f:
            for inp in inputs:
                for p in inp.regex_info.header_parts + inp.regex_info.body_parts:
                    f.write("\t".join(p.captures or []) + "\n")
        r = subprocess.run([exe, caps] + pats + ["--"] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    for tag in ("plain", "regex"):
        lines = [ln.split(" ") for ln in r.stdout.splitlines() if ln.startswith(tag + " ")]
        assert len(lines) == N
        for i, ln in enumerate(lines):
            em = inputs[i].email
            status = A.ZKE_EXTERNAL_INPUT_NULL if i == 3 else A.ZKE_BODY_REGEX_FAIL if (i == 5 and tag == "regex") else A.ZKE_OK
            assert [int(ln[1]), int(ln[2]), int(ln[3])] == [i, status, 0 if tag == "plain" else 1], (tag, i, ln[:4])
            if status != A.ZKE_OK:
                assert ln[4] == "00" * 32 and ln[5] == "", (tag, i)
                continue
            out = A.EmailVerifierOutput(hashlib.sha256(em.from_domain.encode()).digest(), hashlib.sha256(em.public_key.key).digest(), ext_of(i))
            ref = abi_encode(out) if tag == "plain" else abi_encode(out, regex_matches_of(inputs[i]))
            assert ln[5] == ref.hex() and ln[4] == hashlib.sha256(ref).hexdigest(), (tag, i)
