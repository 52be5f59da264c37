"""GPU (-m gpu): the generator half of the C++ host mirror include/zkemail_core.hpp — scan_signatures, select_keys and
generate_email_inputs over a resolver callback — driven through a small compiled program (tests/cpp/sigscan_test.cpp) and
compared with the scan model and the signer's knowledge."""
import subprocess

import pytest

import cases
import sigscan_inputs as I
import sigscan_model as M
from zkemail_rs_amd import _abi as A
from zkemail_rs_amd import build

pytestmark = pytest.mark.gpu


def run(tmp_path, raw, dom, max_sigs, keys=()):
    exe = build.build_cpp_sigscan()
    (tmp_path / "m.eml").write_bytes(raw)
    args = [exe, str(tmp_path / "m.eml"), dom, str(max_sigs)]
    for k, (sel, key, kt) in enumerate(keys):
        (tmp_path / f"k{k}.bin").write_bytes(key)
        args += [sel, str(tmp_path / f"k{k}.bin"), kt]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout.strip().splitlines()


def test_cpp_scan_and_generate(tmp_path):
    raw, dom = I.email_with_signatures(7)
    k0, k1 = cases.K("rsa2048_00"), cases.K("rsa2048_01")
    exp = M.scan_email(raw, dom, 8)
    # good0 verifies under k0; again4 (rsa-sha1, signed by k1) comes later: the resolver knows a wrong key for good0's
    # twin good5 only, so the first candidate's key passes
    rc_, lines = run(tmp_path, raw, dom, 8, [("good0", k0.pkcs1_der, "rsa"), ("again4", k1.pkcs1_der, "rsa")])
    assert lines[0] == f"SCAN {exp.status} {exp.detail} {exp.n_signatures} {exp.n_candidates}"
    assert lines[1:1 + len(exp.sigs)] == [f"SIG {s.header_index} {s.code} {s.algo} {s.selector.decode()} {s.value_span[0]} {s.value_span[1]}" for s in exp.sigs]
    cand = [s.selector.decode() for s in exp.sigs if s.code == 0]
    assert rc_ == 0 and lines[-2] == f"GEN {len(cand)} rsa {len(k0.pkcs1_der)} " + ",".join(f"{dom}/{c}" for c in cand)
    assert lines[-1].startswith("VERIFIED ")
    # the first candidate's fetch fails, a later candidate's key verifies the e-mail (its own signature, rsa-sha1 under k1)
    rc_, lines = run(tmp_path, raw, dom, 8, [("again4", k1.pkcs1_der, "rsa")])
    assert rc_ == 0 and lines[-2].startswith(f"GEN {len(cand)} rsa {len(k1.pkcs1_der)} ")
    # no key at all: "No valid DKIM key found for any signature"; the list cut in front of every candidate; no signature
    rc_, lines = run(tmp_path, raw, dom, 8, [])
    assert rc_ == 1 and lines[-1] == f"PANIC {A.ZKE_DKIM_NOT_PASS} {A.D_KEY_DER} {len(cand)}"
    raw0, _ = I.email_with_signatures(0)
    rc_, lines = run(tmp_path, raw0, dom, 8, [])
    assert rc_ == 1 and lines == ["SCAN 0 0 0 0", f"PANIC {A.ZKE_DKIM_NOT_PASS} {A.D_NO_SIGNATURE} 0"]
    rc_, lines = run(tmp_path, b" x\r\n\r\n", dom, 8, [])
    assert rc_ == 1 and lines == [f"SCAN {A.ZKE_PARSE_FAIL} {A.D_HDR_LEADING_SPACE} 0 0", f"PANIC {A.ZKE_PARSE_FAIL} {A.D_HDR_LEADING_SPACE} 0"]
