"""CPU (-m "not gpu"): the two header splits of csrc/hdrsplit.hip.h as tests/hdr_split_model.py states them, against each
other, against the oracle's zko_parse_headers and against mime_model.parse_headers (string operations, independent of the
oracle's C), on every population of tests/hdr_split_cases.py and on 5 000 seeded structured blocks — and the census of what
each population makes the line-parallel split do.  tests/test_gpu_hdr_split.py runs exactly these populations, so a GPU
test cannot pass while a branch listed here is left out.  Every comparison is for equality."""
import ctypes as C
from collections import Counter

import pytest

from zkemail_rs_amd import _abi as A

import hdr_split_cases as P
import hdr_split_model as H
import mime_model

CODES = {"lead": A.D_HDR_LEADING_SPACE, "lonecr": A.D_HDR_LONE_CR, "many": A.D_U_TOO_MANY_HEADERS}
POPULATIONS = list(P.UNSIGNED) + ["signed"]


def population(name):
    return P.signed()[0] if name == "signed" else P.unsigned(name)


def oracle_split(oracle, raw):
    """zko_parse_headers -> ("ok", spans, the index behind the empty line) | (cause, None, None)"""
    spans = (C.c_uint32 * (4 * A.MAX_HEADERS))()
    body = C.c_size_t()
    n = oracle.lib.zko_parse_headers(raw if raw else b"\0", len(raw), C.addressof(spans), A.MAX_HEADERS, C.byref(body))
    if n < 0:
        return ({v: k for k, v in CODES.items()}[-n], None, None)
    return ("ok", [tuple(spans[4 * i:4 * i + 4]) for i in range(n)], body.value)


def behind_empty_line(raw, hdr_end):
    if raw[hdr_end:hdr_end + 1] == b"\n":
        return hdr_end + 1
    if raw[hdr_end:hdr_end + 2] == b"\r\n":
        return hdr_end + 2
    assert hdr_end == len(raw)
    return hdr_end


def check_against_serial(name, raw, census=None, oracle=None, mime=False):
    ser = H.serial(raw)
    got = H.lines(raw, census)
    assert got is None or got == ser, f"{name}: the line-parallel model {got} differs from the serial walk {ser}"
    if oracle is not None:
        o = oracle_split(oracle, raw)
        if ser[0] == "ok":
            assert o == ("ok", ser[1], behind_empty_line(raw, ser[2])), f"{name}: serial {ser} oracle {o}"
        else:
            assert o == ser, f"{name}: serial {ser} oracle {o}"
    if mime:
        unl = H.serial(raw, max_headers=1 << 30)              # mailparse itself has no limit
        if ser[0] == "many":
            assert unl[0] != "ok" or len(unl[1]) > H.ZKE_MAX_HEADERS, name
        else:
            assert unl == ser, name
        try:
            hs, ix = mime_model.parse_headers(raw)
            m = ("ok", hs, ix)
        except mime_model.MailParseError as e:
            m = ({"leading space": "lead", "lone CR": "lonecr"}[e.what], None, None)
        if unl[0] == "ok":
            want = ("ok", [(raw[a:b], raw[c:d]) for a, b, c, d in unl[1]], behind_empty_line(raw, unl[2]))
            assert m == want, f"{name}: serial {want} mime_model {m}"
        else:
            assert m == unl, f"{name}: serial {unl} mime_model {m}"
    return ser, got


_CENSUS = {}


def census_of(name, oracle):
    if name not in _CENSUS:
        c = Counter()
        results = {}
        for nm, raw, _ in population(name):
            results[nm] = check_against_serial(nm, raw, c, oracle, mime=True)
        _CENSUS[name] = (c, results)
    return _CENSUS[name]


@pytest.mark.parametrize("name", POPULATIONS)
def test_models_oracle_and_mime_model_agree(oracle, name):
    """lines is None or equals serial; serial equals the oracle's split (spans, count, error code, end of the list) and
    mime_model's (keys, values, end of the list); body_offset equals the oracle record's."""
    cs = population(name)
    assert len({nm for nm, _, _ in cs}) == len(cs)
    _, results = census_of(name, oracle)
    key = P.synth.load_keys()["rsa2048_00"].pkcs1_der
    recs = oracle.verify_batch(A.PackedBatch([A.Email(d, raw, A.PublicKey(key)) for _, raw, d in cs]), threads=4)
    for (nm, raw, _), r in zip(cs, recs):
        ser = results[nm][0]
        if ser[0] != "ok":
            want = (A.ZKE_UNSUPPORTED if ser[0] == "many" else A.ZKE_PARSE_FAIL, CODES[ser[0]])
            assert (int(r["status"]), int(r["detail"])) == want, nm
        else:
            assert int(r["status"]) not in (A.ZKE_PARSE_FAIL, A.ZKE_UNSUPPORTED), nm
            assert (int(r["n_headers"]), int(r["body_offset"])) == (len(ser[1]), H.body_offset(raw, ser[2])), nm


def test_census_offset_sweep(oracle):
    c, results = census_of("offset_sweep", oracle)
    assert len(results) == 512 and all(got is not None and got[0] == "ok" for _, got in results.values())
    assert {k[1] for k in c if k[0] == "cut lane"} == set(range(64))           # lanes 62 / 63: the look-ahead is in the next chunk
    assert c[("colon_seen at a chunk edge inside a line", True)] and c[("colon_seen at a chunk edge inside a line", False)]
    # every LF and every first ':' of the tail passes through every lane
    lf_lanes, colon_lanes = set(), set()
    for nm, raw, _ in P.unsigned("offset_sweep"):
        for ks, ke, vs, ve in results[nm][0][1]:
            if raw[ke:ke + 1] == b":":
                colon_lanes.add(ke % 64)
        lf_lanes |= {i % 64 for i in range(results[nm][0][2]) if raw[i] == 10}
    assert lf_lanes == set(range(64)) and colon_lanes == set(range(64))


def test_census_line_counts(oracle):
    c, results = census_of("line_counts", oracle)
    assert c[("vcarry at a group edge", 0)] and c[("vcarry at a group edge", 1)]
    assert c[("value end", "LDS", "a later group than the header start")]
    assert c[("value end", "overflow", "a later group than the header start")]
    assert c[("value end", "overflow", "same group")] and c[("header table", "LDS and overflow")] and c[("header table", "LDS only")]
    for cause in ("lead", "lonecr", "many"):
        assert c[("bad first", cause, "another cause behind")], cause
    assert c[("bad first", "lead", "alone")] and c[("bad first", "lonecr", "alone")]
    assert c[("fallback", "more than LINE_CAP lines")] and not c[("fallback", "no empty line in the staged part")]
    # the named cases do what their names say
    want = {"err_lead_then_257th_header": "lead", "err_257th_header_then_lead": "many", "err_lonecr_then_257th_header": "lonecr",
            "err_257th_header_then_lonecr": "many", "err_lead_then_lonecr": "lead", "err_lonecr_then_lead": "lonecr",
            "err_lead_in_a_later_group_than_lonecr": "lonecr", "lines_257_per1": "many", "lines_513_per1": "many"}
    for nm, cause in want.items():
        assert results[nm][0][0] == cause, nm
    for n in (255, 256):
        assert len(results[f"lines_{n}_per1"][0][1]) == n
    for n in P.LINE_COUNTS:
        assert (results[f"lines_{n}_per3"][1] is None) == (n > H.LINE_CAP), n
        assert results[f"lines_{n}_per3"][0][0] == "ok"
        for edge in (64, 128):
            if n > edge:
                assert results[f"lines_{n}_per3_line{edge}_b_sp_after_keyonly"][0][0] == "lead"
                assert results[f"lines_{n}_per3_line{edge}_a_cont"][0][0] == "ok" and results[f"lines_{n}_per3_line{edge}_c_tab_after_keyonly"][0][0] == "ok"


def test_census_staged_edge(oracle):
    c, results = census_of("staged_edge", oracle)
    assert c[("fallback", "no empty line in the staged part")]
    at = {P_: set() for P_ in P.EDGE_POSITIONS}                # position of the cut LF -> the routes met there
    for nm, raw, _ in P.unsigned("staged_edge"):
        got = "serial" if results[nm][1] is None else "lines"
        assert got == P.STAGED_EDGE_ROUTE[nm] == H.route(raw), nm
        assert results[nm][0][0] == "ok", nm
        if nm.startswith("edge_lf_"):
            at[int(nm.split("_")[2])].add(got)
    # the look-ahead of a cut at 3 566 is staged for an LF empty line (byte 3 567) and is not for a CRLF one (byte 3 568): both
    # routes there, the line path alone in front of it, the serial walk alone behind it
    for P_, routes in at.items():
        assert routes == ({"lines"} if P_ < 3566 else {"lines", "serial"} if P_ == 3566 else {"serial"}), (P_, routes)
    # the DKIM-Signature header placed at the edge: its ':' / fold LF / value end is where the name says
    for nm, raw, _ in P.unsigned("staged_edge"):
        for what in ("colon", "fold", "value_end"):
            if nm.startswith(f"edge_{what}_"):
                pos = int(nm.rsplit("_", 1)[1])
                ks, ke, vs, ve = [sp for sp in results[nm][0][1] if raw[sp[0]:sp[1]] == b"DKIM-Signature"][-1]
                assert {"colon": ke, "fold": raw.index(b"\n", vs), "value_end": ve}[what] == pos, nm


def test_census_short_inputs(oracle):
    c, results = census_of("short_inputs", oracle)
    assert len(results) == 1 + 6 + 36 + 216 + 22
    assert c["empty input"] == 1 and c["empty list"] and c[("fallback", "no empty line in the staged part")]
    assert {r[0][0] for r in results.values()} == {"ok", "lead", "lonecr"}
    assert any(got is not None and got[0] != "ok" for _, got in results.values())     # errors met on the line path too


def test_census_find_body(oracle):
    _, results = census_of("find_body", oracle)
    dist = set()
    for nm, raw, _ in P.unsigned("find_body"):
        ser = results[nm][0]
        assert ser[0] == "ok" and len(ser[1]) == 3, nm
        off = H.body_offset(raw, ser[2])
        if "_d" in nm:
            dist.add(off - 4 - ser[2])
            assert off - 4 - ser[2] == int(nm.rsplit("_d", 1)[1]), nm
        if nm.endswith("_none") or nm.endswith("_crlfcr_last_three"):
            assert off == len(raw), nm
        if nm.endswith("_last_four"):
            assert off == len(raw) and raw.endswith(b"\r\n\r\n") and raw.count(b"\r\n\r\n") == 1, nm
    assert dist == set(range(131))


def test_census_signed(oracle):
    c, results = census_of("signed", oracle)
    cs, emails, inter, sig_index, routes = P.signed()
    assert len(cs) == 2 * (3 * 48 + 11 + 8)
    lanes = {r: set() for r in ("L", "S-hbm", "S-lds", "S-hbm-later")}
    entries = set()
    for (nm, raw, _), rt in zip(cs, routes):
        ser, got = results[nm]
        assert ser[0] == "ok" and (got is None) == (rt in ("S-hbm", "S-hbm-later")), nm
        if "_behind_" not in nm:
            lanes[rt].add((ser[2] - 1) % 64)
        names = [raw[a:b].lower() for a, b, _, _ in ser[1]]
        assert names.count(b"dkim-signature") == (2 if rt in ("S-lds", "S-hbm-later") else 1), nm
        if "_behind_" in nm:
            entries |= {i for i, k in enumerate(names) if k in (b"from", b"to", b"subject", b"date", b"message-id")}
    assert all(len(v) >= (11 if r == "S-hbm-later" else 48) for r, v in lanes.items()), {k: len(v) for k, v in lanes.items()}     # 48 shifts, two cores of unlike length
    assert {62, 63, 64, 65, 66} <= entries


def test_structured_blocks(oracle):
    """5 000 seeded blocks of the populations' line kinds: long valid blocks, which byte mutation never builds."""
    c = Counter()
    outcome = Counter()
    for nm, raw, _ in P.structured_blocks():
        ser, got = check_against_serial(nm, raw, c, oracle)
        outcome[(ser[0], "serial" if got is None else "lines")] += 1
        if ser[0] == "ok":
            outcome["more than 64 headers"] += len(ser[1]) > 64
    assert outcome[("ok", "lines")] > 2000 and outcome["more than 64 headers"] > 1000, outcome
    for k in (("ok", "serial"), ("lead", "lines"), ("lonecr", "lines"), ("many", "lines"), ("many", "serial")):
        assert outcome[k] > 10, outcome
    assert c[("vcarry at a group edge", 0)] > 100 and c[("vcarry at a group edge", 1)] > 100
    assert c[("value end", "overflow", "a later group than the header start")] > 100
    assert c[("fallback", "more than LINE_CAP lines")] > 10 and c[("fallback", "no empty line in the staged part")] > 10
