"""-m gpu: the header split of csrc/hdrsplit.hip.h (split_headers_lines, scan_headers behind it and in later signature rounds,
find_body) on the populations of tests/hdr_split_cases.py, one batch per population and entry.  The verify entry is compared
with the oracle record for record and with tests/hdr_split_model.py (header count, body offset, which error); the scan entry
with tests/sigscan_model.py, and the header index and value span of every header named DKIM-Signature with the model's span
of that header — a span of the split read off the device directly; the signed population with the Python signer.  Every
comparison is against the CPU.  tests/test_hdr_split_model.py certifies what each population reaches."""
import numpy as np
import pytest

from zkemail_rs_amd import _abi as A

import hdr_split_cases as P
import hdr_split_model as H
import sigscan_model as M
import synth
from test_gpu_sigscan import assert_scans_equal
from test_gpu_verify import assert_records_equal, run_both

pytestmark = pytest.mark.gpu

CODES = {"lead": (A.ZKE_PARSE_FAIL, A.D_HDR_LEADING_SPACE), "lonecr": (A.ZKE_PARSE_FAIL, A.D_HDR_LONE_CR),
         "many": (A.ZKE_UNSUPPORTED, A.D_U_TOO_MANY_HEADERS)}
POPULATIONS = list(P.UNSIGNED) + ["signed"]
_MODEL = {}


def population(name):
    return P.signed()[0] if name == "signed" else P.unsigned(name)


def model(name):
    """name of the population -> serial(raw) of each case, computed once"""
    if name not in _MODEL:
        _MODEL[name] = [H.serial(raw) for _, raw, _ in population(name)]
    return _MODEL[name]


@pytest.mark.parametrize("name", list(P.UNSIGNED))
def test_verify_entry(engine, oracle, name):
    cs = population(name)
    key = A.PublicKey(synth.load_keys()["rsa2048_00"].pkcs1_der)
    got, exp, _, _ = run_both(engine, oracle, [A.Email(d, raw, key) for _, raw, d in cs], dbg=False)
    names = [nm for nm, _, _ in cs]
    assert_records_equal(got, exp, names, name)
    for (nm, raw, _), g, ser in zip(cs, got, model(name)):
        if ser[0] != "ok":
            assert (int(g["status"]), int(g["detail"])) == CODES[ser[0]], nm
        else:
            assert (int(g["status"]), int(g["detail"])) not in CODES.values(), nm
            assert (int(g["n_headers"]), int(g["body_offset"])) == (len(ser[1]), H.body_offset(raw, ser[2])), nm


@pytest.mark.parametrize("name", POPULATIONS)
def test_scan_entry(engine, name):
    cs = population(name)
    raws, doms = [raw for _, raw, _ in cs], [d for _, _, d in cs]
    pairs = list(zip(raws, doms))
    got = engine.scan_signatures(raws, doms, A.SCAN_MAX_SIGS)
    assert_scans_equal(got, M.scan(raws, doms, A.SCAN_MAX_SIGS), pairs, name)
    listed = 0
    for (nm, raw, _), g, ser in zip(cs, got, model(name)):
        if ser[0] != "ok":
            assert (g.status, g.detail) == CODES[ser[0]] and not g.sigs, nm
            continue
        named = [(hx, (vs, ve)) for hx, (ks, ke, vs, ve) in enumerate(ser[1]) if raw[ks:ke].lower() == b"dkim-signature"]
        assert g.status == A.ZKE_OK and g.n_signatures == len(named) <= A.SCAN_MAX_SIGS, nm
        assert [(s.header_index, tuple(s.value_span)) for s in g.sigs] == named, nm
        listed += len(named)
    assert listed >= (0 if name == "short_inputs" else len(cs)), name          # spans were read: the equality is not vacuous


def test_signed_population(engine, oracle):
    """Every e-mail verifies: the header preimage is the signer's byte for byte, both hashes are the signer's, and the
    signature that verified is the first (routes L and S-hbm) or the second (S-lds and S-hbm-later, found by the later round's
    serial walk)."""
    cs, emails, inter, sig_index, routes = P.signed()
    got, exp, d1, _ = run_both(engine, oracle, emails)
    names = [nm for nm, _, _ in cs]
    assert_records_equal(got, exp, names, "signed")
    for i, (nm, it) in enumerate(zip(names, inter)):
        assert int(got[i]["status"]) == A.ZKE_OK, f"{nm}: {int(got[i]['status'])}/{int(got[i]['detail'])}"
        pre = it["canon_header"]
        assert int(got[i]["canon_header_len"]) == len(pre) and bytes(d1.canon_header[i, :len(pre)]) == pre, nm
        assert bytes(got[i]["body_hash"]) == it["body_hash"] and bytes(got[i]["header_hash"]) == it["header_hash"], nm
        assert int(got[i]["sig_index"]) == sig_index[i], nm
    assert {r: routes.count(r) for r in set(routes)} == {"L": 2 * 48 + 16, "S-hbm": 2 * 48, "S-lds": 2 * 48, "S-hbm-later": 2 * 11}
    assert not np.asarray(got["status"]).any()
