"""GPU (-m gpu): the key-record part of the C++ host mirror include/zkemail_core.hpp — decode_key_records and
generate_email_inputs_from_records over a resolver callback — driven through a small compiled program (tests/cpp/keyrec_test.cpp)
and compared with the key-record model and the published keys of RFC 8463."""
import hashlib
import subprocess

import pytest

import keyrec_cases as K
import keyrec_model as M
import test_rfc8463_vector as V
from zkemail_rs_amd import _abi as A
from zkemail_rs_amd import build

pytestmark = pytest.mark.gpu


def run(tmp_path, mode, raw, dom, records=()):
    exe = build.build_cpp_keyrec()
    (tmp_path / "m.eml").write_bytes(raw)
    args = [exe, str(mode), str(tmp_path / "m.eml"), dom]
    for k, (sel, rec) in enumerate(records):
        (tmp_path / f"r{k}.txt").write_bytes(rec)
        args += [sel, str(tmp_path / f"r{k}.txt")]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout.strip().splitlines()


def key_lines(records, mode):
    out = []
    for x in M.decode_all([r for _, r in records] + [b""], mode):
        out.append("KEY %d %d %d %s" % (x.code, x.key_type, len(x.key), (x.key[:2] + b"\0\0")[:2].hex()))
    return out


@pytest.mark.parametrize("mode", [M.ARCHIVE, M.DNS])
def test_cpp_decode_and_generate_from_records(tmp_path, mode):
    r = K.rfc8463()
    ed = (r["ed25519"]["selector"], b"v=DKIM1; k=ed25519; p=" + r["ed25519"]["p_base64"].encode())
    rsa = (r["rsa"]["selector"], b"v=DKIM1; k=rsa; p=" + r["rsa"]["p_base64_spki"].encode())
    bad = ("unused", b"v=DKIM1; k=rsa; p=AAAA")
    # both records known: the Ed25519 signature is the first header, its key is chosen
    rc_, lines = run(tmp_path, mode, V.RAW, V.DOMAIN, [ed, rsa, bad])
    assert lines[:4] == key_lines([ed, rsa, bad], mode)
    assert rc_ == 0 and lines[4] == "GEN 2 ed25519 32" and lines[5] == "VERIFIED " + hashlib.sha256(V.ED_KEY.key).digest()[:2].hex()
    # the Ed25519 record withheld: the RSA key, re-encoded as PKCS#1 on the device
    rc_, lines = run(tmp_path, mode, V.RAW, V.DOMAIN, [rsa])
    assert lines[:2] == key_lines([rsa], mode)
    assert rc_ == 0 and lines[2] == f"GEN 2 rsa {len(V.RSA_KEY.key)}" and lines[3] == "VERIFIED " + hashlib.sha256(V.RSA_KEY.key).digest()[:2].hex()
    # an undecodable record for every selector: "No valid DKIM key found for any signature"
    rc_, lines = run(tmp_path, mode, V.RAW, V.DOMAIN, [(ed[0], bad[1]), (rsa[0], b"v=DKIM1; p=")])
    assert rc_ == 1 and lines[-1] == f"PANIC {A.ZKE_DKIM_NOT_PASS} {A.D_KEY_DER} 2"
