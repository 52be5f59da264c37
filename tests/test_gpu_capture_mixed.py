"""GPU (-m gpu): zke_extract_captures_mixed — the extraction over e-mails that carry different regex configs, and e-mails without
one, in ONE batch.  Expectations (tests/capture_mixed_cases.py): records from the oracle over inputs built from Python `re`
captures, strings and spans from `re`, origins from tests/qp_map_model.py; group-missing and capture-limit verdicts, which the
oracle cannot express, as hand-derived (status, detail, regex_part, match_count).  Cases 1 to 3 run under dfa_mapping 1 and 2."""
import ctypes as C
import re
import threading

import numpy as np
import pytest

import capture_mixed_cases as cx
import capture_model
import mixed_cases as mc
import qp_map_model as Q
import zkemail_rs_amd as z
from zkemail_rs_amd import _abi as A
from zkemail_rs_amd import regex_compile as rc

pytestmark = pytest.mark.gpu

MAPPINGS = [1, 2]
E_ARG, E_NOMEM = -1, -3
CYCLE = ["A", "B", None, "C", "D", "NINE", "THREE"]


@pytest.fixture(scope="module")
def engines():
    return {1: z.Engine(dfa_mapping=1), 2: z.Engine(dfa_mapping=2)}


def assignment(names, n, start=0):
    """n pool e-mails in turn, names cyclically: (pool indices, config names, e-mails, the oracle's inputs)."""
    ix = [start + k for k in range(n)]
    keys = [names[k % len(names)] for k in range(n)]
    return ix, keys, [mc.pool()[k % mc.POOL_N].email for k in ix], [cx.oracle_input(k, name) for k, name in zip(ix, keys)]


@pytest.fixture(scope="module")
def case1(oracle):
    """[A, B, None, C, D, NINE, THREE] cyclically over 56 pool e-mails (7 is coprime to the pool's period of 8: each config meets
    every pool kind), the oracle's records, and the non-vacuity of the case — asserted before any engine is looked at."""
    ix, keys, emails, inputs = assignment(CYCLE, 56)
    exp = mc.expectation(oracle, inputs, keys)
    mc.check_not_vacuous(exp, keys, False)                                                      # every populated config has an OK e-mail
    failing = {k for i, k in enumerate(keys) if k is not None and int(exp[i]["status"]) in mc.REGEX_STAGE}
    assert len(failing) >= 3, failing
    assert any(k is not None and int(exp[i]["status"]) == A.ZKE_DKIM_NOT_PASS for i, k in enumerate(keys))
    split = 0
    for i, (k, name) in enumerate(zip(ix, keys)):
        if name is not None and int(exp[i]["status"]) == A.ZKE_OK and (k % mc.POOL_N) % 3 == 0:      # a QP e-mail
            hp, bp = cx.catalogue(name)
            cols = cx.model_origins(oracle, mc.pool()[k % mc.POOL_N], name)
            col = sum(len(g) for _, g in hp)
            for pat, g in bp:
                if pat == mc.B_ORDER[0]:
                    split += cols[col][2] == Q.ORGF_SPLIT
                col += len(g)
    assert split >= 1
    return ix, keys, emails, exp


@pytest.mark.parametrize("mapping", MAPPINGS)
def test_every_config_at_once(engines, oracle, case1, mapping):
    ix, keys, emails, exp = case1
    x = cx.Extraction(engines[mapping], emails, keys, origins=True)
    mc.assert_equal(x.out, exp, "case 1")
    cx.check_against_re(x, oracle, ix, keys, exp, origins=True, ctx="case 1")
    plain = [i for i, k in enumerate(keys) if k is None]
    rec = oracle.verify_batch(A.PackedBatch([emails[i] for i in plain]), threads=4)
    mc.assert_equal(x.out[plain], rec, "e-mails without a config")
    # the Python keyword delivers the same: a RegexInfo for the OK e-mails with a config, ragged origins
    recs, infos, (osp, ofl) = engines[mapping].extract_captures_mixed(emails, [cx.regex_config(k) for k in keys], unicode=False, origins=True)
    assert recs.tobytes() == x.out.tobytes()
    for i, k in enumerate(keys):
        ok = k is not None and int(exp[i]["status"]) == A.ZKE_OK
        assert (infos[i] is not None) == ok, i
        assert osp[i].shape == (int(x.lists.col_off[i + 1] - x.lists.col_off[i]), 2) and (osp[i] == x.columns(i)[2]).all() and (ofl[i] == x.columns(i)[3]).all()
        if ok:
            want = mc.parts_for(mc.pool()[ix[i] % mc.POOL_N], cx.catalogue(k))
            got = [p.captures for p in (infos[i].header_parts or []) + (infos[i].body_parts or [])]
            assert got == [p.captures for p in (want.header_parts or []) + (want.body_parts or [])], i
            assert (infos[i].header_parts is None) == (want.header_parts is None) and (infos[i].body_parts is None) == (want.body_parts is None)


@pytest.mark.parametrize("mapping", MAPPINGS)
def test_round_trip_into_verify_mixed(engines, oracle, case1, mapping):
    """The tables of case 1 go verbatim, with the DFA ids, into zke_verify_emails_mixed.  An e-mail whose extraction failed carries
    no strings, and its match count (or DKIM) fails before any containment test: the records are the oracle's of case 1."""
    eng = engines[mapping]
    ix, keys, emails, exp = case1
    x = cx.Extraction(eng, emails, keys, origins=False)
    ml = cx.verify_mixed_lists(x)
    assert list(ml.job_off) == list(x.lists.job_off)
    got = np.zeros(len(emails), dtype=A.RESULT_DTYPE)
    assert eng.lib.zke_verify_emails_mixed(eng.h, x.refs.arr, x.refs.n, C.byref(ml.c), got.ctypes.data) == 0, eng.lib.zke_last_error(eng.h)
    mc.assert_equal(got, exp, "round trip")
    ok = [i for i in range(len(emails)) if int(exp[i]["status"]) == A.ZKE_OK]
    cfgs = [cx.regex_config(k) for k in keys]
    values = z.generate_email_with_regex_inputs_mixed([emails[i] for i in ok], [cfgs[i] for i in ok], unicode=False, engine=eng)
    assert [isinstance(v, A.Email) for v in values] == [keys[i] is None for i in ok]
    rec = eng.verify_emails_mixed(values)
    assert (rec["status"] == A.ZKE_OK).all()
    bad = next(i for i in range(len(emails)) if keys[i] is not None and int(exp[i]["status"]) != A.ZKE_OK)
    with pytest.raises(z.VerifyPanic):
        z.generate_email_with_regex_inputs_mixed([emails[i] for i in ok[:3] + [bad]], [cfgs[i] for i in ok[:3] + [bad]], unicode=False, engine=eng)


def run_and_check(eng, oracle, names, n, ctx, start=0, lists=None, keys_for_lists=None):
    ix, keys, emails, inputs = assignment(names, n, start)
    exp = mc.expectation(oracle, inputs, keys)
    x = cx.Extraction(eng, emails, keys, origins=True, lists=lists)
    mc.assert_equal(x.out, exp, ctx)
    cx.check_against_re(x, oracle, ix, keys, exp, origins=True, ctx=ctx)
    return x, exp, keys


@pytest.mark.parametrize("mapping", MAPPINGS)
def test_shapes_at_the_edges(engines, oracle, mapping):
    eng = engines[mapping]
    # n = 0 returns 0
    lists0 = A.CaptureMixedLists([], [])
    o = A.zke_capture_out()
    one = np.zeros(4, np.uint32)
    o.spans, o.flags, o.cap_off, o.cap_off_cap, o.cap_str_off, o.cap_str_off_cap = one.ctypes.data, one.ctypes.data, one.ctypes.data, 1, one.ctypes.data + 8, 1
    assert eng.lib.zke_extract_captures_mixed(eng.h, None, 0, C.byref(lists0.c), None, C.byref(o), None) == 0
    # n = 1: an e-mail with a config, an e-mail without
    x, exp, _ = run_and_check(eng, oracle, ["B"], 1, "n=1")
    assert int(exp[0]["status"]) == A.ZKE_OK and x.lists.J == 3 and x.lists.Gt == 3
    run_and_check(eng, oracle, [None], 1, "n=1 no config")
    # all ZKE_CONFIG_NONE: no job, no column, no string
    x, exp, _ = run_and_check(eng, oracle, [None], 16, "all none")
    assert x.lists.J == 0 and x.lists.Gt == 0 and list(x.cap_off) == [0] and list(x.cap_str_off) == [0] and A.ZKE_OK in set(exp["status"])
    # K = 1: one config for all — and what the single-config entry gives the same batch
    x, exp, keys = run_and_check(eng, oracle, ["NINE"], 24, "K=1")
    recs, infos = eng.extract_captures([mc.pool()[k].email for k in range(24)], cx.regex_config("NINE"), unicode=False)
    mc.assert_equal(x.out, recs, "K=1 against the single-config entry")
    # an unpopulated config between two populated ones
    ix, keys, emails, inputs = assignment(["A", "D"], 24)
    packed, _ = eng.pack_capture_mixed([cx.regex_config(k) for k in ("A", "NINE", "D")], unicode=False)
    lists = A.CaptureMixedLists(packed.configs, [0 if k == "A" else 2 for k in keys])
    x, exp, _ = run_and_check(eng, oracle, ["A", "D"], 24, "unpopulated config", lists=lists)
    assert {A.ZKE_OK, A.ZKE_DKIM_NOT_PASS} <= set(int(s) for s in exp["status"])
    # a config with no requested group at all next to one with two groups in one part
    x, exp, keys = run_and_check(eng, oracle, ["GZERO", "TWO", None], 48, "G = 0 beside two groups in a part")
    assert all(x.lists.col_off[i] == x.lists.col_off[i + 1] for i, k in enumerate(keys) if k == "GZERO")
    assert any(k == "GZERO" and int(exp[i]["status"]) == A.ZKE_OK for i, k in enumerate(keys))
    assert any(k == "GZERO" and int(exp[i]["status"]) == A.ZKE_HEADER_REGEX_FAIL for i, k in enumerate(keys))        # two Subject headers
    assert any(k == "TWO" and int(exp[i]["status"]) == A.ZKE_OK and len(x.strings(i)[0]) == 2 for i, k in enumerate(keys))
    # the same pattern a header part in one config and a body part in another (pool e-mails 2, 10, 18 carry the marker in the Subject)
    x, exp, keys = run_and_check(eng, oracle, ["ORDER_IN_HEADER", "D"], 24, "header and body", start=2)
    assert x.lists.configs[0][0][0][:2] == x.lists.configs[1][1][0][:2]                # one pair, one program, on both sides
    assert {int(exp[i]["status"]) for i in range(0, 24, 2)} >= {A.ZKE_OK, A.ZKE_HEADER_REGEX_FAIL}


def test_workspace_rows_and_the_looping_wave(engine, oracle):
    """A program of more than CAP_LDS_STATES states (rows in the slot's workspace, the grid bounded by CAP_WORK_WAVES) in one config,
    small programs in another, more jobs than waves: every wave takes more than one item."""
    pat = cx.BIG_ORDER[0]
    prog = rc.create_capture_program(pat, unicode=False)
    assert cx.CAP_LDS_STATES < int.from_bytes(prog[8:12], "little") <= A.CAP_MAX_STATES
    m0 = mc.pool()[0]
    ms = list(re.finditer(pat.encode(), m0.clean_body))
    assert len(ms) == 1
    slots = capture_model.captures_at(capture_model.Program(prog), m0.clean_body, ms[0].start())
    assert (slots[0], slots[1], slots[2], slots[3]) == (*ms[0].span(), *ms[0].span(1))
    ix, keys, emails, inputs = assignment(["BIGNINE", "A"], 64)
    exp = mc.expectation(oracle, inputs, keys)
    x = cx.Extraction(engine, emails, keys, origins=True)
    assert x.lists.J == 32 * 9 + 32 * 2 > cx.CAP_WORK_WAVES
    assert sum(1 for i, k in enumerate(keys) if k == "BIGNINE" and int(exp[i]["status"]) == A.ZKE_OK) >= 8
    mc.assert_equal(x.out, exp, "workspace rows")
    cx.check_against_re(x, oracle, ix, keys, exp, origins=True, ctx="workspace rows")


def test_one_fold_per_email_with_its_own_config(engine, oracle):
    """Config X asks the from pattern for a group it lacks in part 0, config Y has the subject pattern first: Y's twosubj e-mails
    report the match count of part 0, X's e-mails (those that pass DKIM: a bad signature is reported first) the missing group of
    part 0 — and neither verdict leaks into the other config's e-mails."""
    names = ["X_MISSING", "Y_SUBJ_FIRST", "X_MISSING"]       # period 3: both configs meet every pool kind
    ix = list(range(48))
    keys = [names[k % 3] for k in ix]
    emails = [mc.pool()[k % mc.POOL_N].email for k in ix]
    # the oracle knows Y (X's group cannot be written down as a capture string); for X it gives the DKIM verdicts
    exp = np.zeros(48, dtype=A.RESULT_DTYPE)
    ys = [i for i in ix if keys[i] == "Y_SUBJ_FIRST"]
    exp[ys] = mc.expectation(oracle, [cx.oracle_input(ix[i], keys[i]) for i in ys], [keys[i] for i in ys])
    dkim = oracle.verify_batch(A.PackedBatch(emails), threads=4)
    x = cx.Extraction(engine, emails, keys, origins=False)
    seen = set()
    for i, (k, name) in enumerate(zip(ix, keys)):
        r, kind = x.out[i], mc.pool()[k % mc.POOL_N].kind
        got = (int(r["status"]), int(r["detail"]), int(r["regex_part"]), int(r["match_count"]))
        if kind == "badsig":
            assert int(dkim[i]["status"]) == A.ZKE_DKIM_NOT_PASS
            assert (got[0], got[1]) == (int(dkim[i]["status"]), int(dkim[i]["detail"])), (i, got)
        elif name == "X_MISSING":
            assert got == (A.ZKE_HEADER_REGEX_FAIL, A.D_RE_GROUP_MISSING, 0, 1), (i, got)
        elif kind == "twosubj":
            assert got == (A.ZKE_HEADER_REGEX_FAIL, A.D_RE_MATCH_COUNT, 0, 2), (i, got)
            mc.assert_equal(x.out[i:i + 1], exp[i:i + 1], f"twosubj {i}")
        else:
            assert int(exp[i]["status"]) == A.ZKE_OK
            mc.assert_equal(x.out[i:i + 1], exp[i:i + 1], f"Y {i}")
        seen.add((name, kind))
        if got[0] != A.ZKE_OK:
            assert all(s == [] for s in x.strings(i)) and (x.columns(i)[0] == cx.NONE).all()
    assert {("X_MISSING", "twosubj"), ("Y_SUBJ_FIRST", "twosubj"), ("X_MISSING", "plain"), ("Y_SUBJ_FIRST", "plain"), ("X_MISSING", "badsig")} <= seen
    for i, name in enumerate(keys):                     # Y's OK e-mails deliver their strings
        if name == "Y_SUBJ_FIRST" and int(exp[i]["status"]) == A.ZKE_OK:
            assert x.strings(i) == [w[0] for w in cx.re_captures(mc.pool()[ix[i] % mc.POOL_N], name)]


def test_bad_ids_stay_local(engine, oracle):
    """An unregistered program id in one config, a junk DFA pair in another: their e-mails fail, the others are as in case 1."""
    names = ["A", "BADPROG", "B", "JUNK"]
    ix = list(range(48))
    keys = [names[k % 4] for k in ix]
    emails = [mc.pool()[k % mc.POOL_N].email for k in ix]
    packed, _ = engine.pack_capture_mixed([cx.regex_config(k) for k in ("A", "B")], unicode=False)
    _, from_dfa, _ = engine.compile_pattern(mc.H_FROM[0], False)
    junk = engine.dfa_register(b"junk", b"junk")
    _, _, from_prog = engine.compile_pattern(mc.H_FROM[0], False)
    configs = [packed.configs[0], ([(from_dfa, 0x7FFFFFF0, [1])], []), packed.configs[1], ([(junk, from_prog, [1])], [])]
    lists = A.CaptureMixedLists(configs, [names.index(k) for k in keys])
    good = [i for i, k in enumerate(keys) if k in ("A", "B")]
    exp = mc.expectation(oracle, [cx.oracle_input(ix[i], keys[i]) for i in good], [keys[i] for i in good])
    dkim = oracle.verify_batch(A.PackedBatch(emails), threads=4)
    x = cx.Extraction(engine, emails, keys, origins=False, lists=lists)
    mc.assert_equal(x.out[good], exp, "the remaining configs")
    assert A.ZKE_OK in set(int(s) for s in exp["status"])
    hit = set()
    for i, k in enumerate(keys):
        r = x.out[i]
        if k in ("A", "B"):
            if int(r["status"]) == A.ZKE_OK:
                assert x.strings(i) == [w[0] for w in cx.re_captures(mc.pool()[ix[i] % mc.POOL_N], k)]
            continue
        if int(dkim[i]["status"]) != A.ZKE_OK:
            assert int(r["status"]) == int(dkim[i]["status"]) and int(r["detail"]) == int(dkim[i]["detail"])
            continue
        if k == "BADPROG":
            assert (int(r["status"]), int(r["detail"]), int(r["regex_part"]), int(r["match_count"])) == (A.ZKE_UNSUPPORTED, A.D_U_CAPTURE_PROGRAM, 0, 1), i
        else:
            assert int(r["status"]) == A.ZKE_DFA_DECODE_FAIL and int(r["detail"]) != 0, i
        assert x.strings(i) == [[]] and (x.columns(i)[0] == cx.NONE).all()
        hit.add(k)
    assert hit == {"BADPROG", "JUNK"}


def raw_call(eng, refs, lists, sizes, blob_cap, out=None, org_sizes=None):
    """One zke_extract_captures_mixed with buffers of exactly `sizes` = (spans, flags, cap_off, cap_str_off) entries."""
    bufs = [np.full(max(s, 1), 0x5A5A5A5A, np.uint32) for s in (sizes[0], 1, sizes[2], sizes[3])]
    fl = np.full(max(sizes[1], 1), 0x5A, np.uint8)
    blob = np.full(max(blob_cap, 1), 0x5A, np.uint8)
    o = A.zke_capture_out()
    o.spans, o.spans_cap, o.flags, o.flags_cap = bufs[0].ctypes.data, sizes[0], fl.ctypes.data, sizes[1]
    o.cap_off, o.cap_off_cap, o.cap_str_off, o.cap_str_off_cap = bufs[2].ctypes.data, sizes[2], bufs[3].ctypes.data, sizes[3]
    o.cap_blob, o.cap_blob_cap = blob.ctypes.data, blob_cap
    for f in ("spans_need", "flags_need", "cap_off_need", "cap_str_off_need", "cap_blob_need", "n_strings"):
        setattr(o, f, 0xABCD)
    out = np.full(max(refs.n, 1), 0x5A, dtype=np.uint8).repeat(A.RESULT_DTYPE.itemsize).view(A.RESULT_DTYPE) if out is None else out
    org = None
    if org_sizes is not None:
        org = A.zke_capture_origin()
        os_, of_ = np.zeros(max(org_sizes[0], 1), np.uint32), np.zeros(max(org_sizes[1], 1), np.uint8)
        org.spans, org.spans_cap, org.flags, org.flags_cap = os_.ctypes.data, org_sizes[0], of_.ctypes.data, org_sizes[1]
        bufs += [os_, of_]
    rc_ = eng.lib.zke_extract_captures_mixed(eng.h, refs.arr, refs.n, C.byref(lists.c), out.ctypes.data, C.byref(o), C.byref(org) if org is not None else None)
    return rc_, o, org, out, (bufs[0], fl, bufs[2], bufs[3], blob)


def test_buffer_protocol(engine, oracle):
    ix, keys, emails, inputs = assignment(CYCLE, 28)
    lists, _ = engine.pack_capture_mixed([cx.regex_config(k) for k in keys], unicode=False)
    refs = A.EmailRefs(emails)
    J, Gt = lists.J, lists.Gt
    full = (2 * Gt, Gt, J + 1, Gt + 1)
    for short in range(4):                                   # a fixed-size buffer one entry short: at once, every *_need by the formulas
        sizes = tuple(s - (k == short) for k, s in enumerate(full))
        rc_, o, _, out, _ = raw_call(engine, refs, lists, sizes, 4096)
        assert rc_ == E_NOMEM and (o.spans_need, o.flags_need, o.cap_off_need, o.cap_str_off_need) == full, short
        assert (out.view(np.uint8) == 0x5A).all()
    for short in range(2):                                   # the origins likewise
        rc_, o, org, out, _ = raw_call(engine, refs, lists, full, 4096, org_sizes=(2 * Gt - (short == 0), Gt - (short == 1)))
        assert rc_ == E_NOMEM and (org.spans_need, org.flags_need) == (2 * Gt, Gt)
    ref = cx.Extraction(engine, emails, keys, origins=False, lists=lists)
    need = len(ref.blob)
    assert need > 0
    rc_, o, _, out, (spans, fl, cap_off, cap_str_off, blob) = raw_call(engine, refs, lists, full, need - 1)
    assert rc_ == E_NOMEM and o.cap_blob_need == need and o.n_strings == len(ref.cap_str_off) - 1
    assert out.tobytes() == ref.out.tobytes() and (spans[:2 * Gt].reshape(Gt, 2) == ref.spans).all() and (fl[:Gt] == ref.flags).all()
    assert (cap_off == ref.cap_off).all() and (cap_str_off[:o.n_strings + 1] == ref.cap_str_off).all()
    rc_, o, _, out, (_, _, _, _, blob) = raw_call(engine, refs, lists, full, int(o.cap_blob_need))
    assert rc_ == 0 and blob[:need].tobytes() == ref.blob.tobytes()


def test_argument_errors_leave_the_outputs_untouched(engine):
    """Every ZKE_E_ARG condition of the header, refused before anything is staged: `out` and `caps` are as they were."""
    m = mc.pool()[0].email
    _, d, p = engine.compile_pattern(mc.H_FROM[0], False)
    part = (d, p, [1])

    def refused(lists, n=2, tweak=None):
        refs = A.EmailRefs([m] * n)
        if tweak:
            tweak(lists)
        rc_, o, _, out, bufs = raw_call(engine, refs, lists, (64, 64, 64, 64), 64)
        assert rc_ == E_ARG, rc_
        assert (out.view(np.uint8) == 0x5A).all() and all((b.view(np.uint8) == 0x5A).all() for b in bufs)
        assert [getattr(o, f) for f in ("spans_need", "flags_need", "cap_off_need", "cap_str_off_need", "cap_blob_need", "n_strings")] == [0xABCD] * 6

    ok = lambda: A.CaptureMixedLists([([part], [])], [0, 0])
    refused(A.CaptureMixedLists([([part], [])] * (A.MIXED_MAX_CONFIGS + 1), [0, 0]))                 # too many configs
    refused(A.CaptureMixedLists([([], [])], [0, 0]))                                                # a config with 0 parts
    refused(A.CaptureMixedLists([([part] * 9, [part] * 8)], [0, 0]))                                # 17 parts
    refused(A.CaptureMixedLists([([(d, p, [0] * (A.CAP_MAX_GROUPS + 1))], [])], [0, 0]))            # 17 groups in a part
    refused(ok(), tweak=lambda L: setattr(L.c, "configs", None))                                    # null lists with a count
    refused(ok(), tweak=lambda L: setattr(L.arr[0], "header_parts", None))
    refused(ok(), tweak=lambda L: setattr(L.arr[0].header_parts[0], "groups", None))
    refused(ok(), tweak=lambda L: setattr(L.c, "config_of", None))
    refused(A.CaptureMixedLists([([part], [])], [0, 0]), tweak=lambda L: L.config_of.__setitem__(1, 1))     # config_of names no config
    big = A.CaptureMixedLists([([(d, p, [0] * 16)] * 16, [])], [0] * 4096)                          # Gt = 2^20: refused before staging
    assert big.Gt == 1 << 20
    refused(big, n=4096)


def test_asynchronous_use_on_four_slots(oracle):
    """Two host threads on one engine with four slots, ten iterations each: one issues mixed extractions, the other
    zke_verify_emails_mixed of the same inputs; every result equals the serial run's."""
    eng = z.Engine(slots=4)
    try:
        ix, keys, emails, inputs = assignment(CYCLE, 42)
        chunks = [slice(0, 21), slice(21, 42)]
        cfgs = [cx.regex_config(k) for k in keys]
        serial_x = [eng.extract_captures_mixed(emails[c], cfgs[c], unicode=False, origins=True) for c in chunks]
        serial_v = [eng.verify_emails_mixed(inputs[c]) for c in chunks]
        mc.assert_equal(np.concatenate([s[0] for s in serial_x]), mc.expectation(oracle, inputs, keys), "serial")
        got, errors = {}, []

        def extractor():
            try:
                for rep in range(10):
                    got[("x", rep)] = eng.extract_captures_mixed(emails[chunks[rep % 2]], cfgs[chunks[rep % 2]], unicode=False, origins=True)
            except Exception as e:                                # noqa: BLE001
                errors.append(e)

        def verifier():
            try:
                for rep in range(10):
                    got[("v", rep)] = eng.verify_emails_mixed(inputs[chunks[rep % 2]])
            except Exception as e:                                # noqa: BLE001
                errors.append(e)

        ts = [threading.Thread(target=extractor), threading.Thread(target=verifier)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors
        for rep in range(10):
            rx, ix_, (osp, ofl) = got[("x", rep)]
            sx = serial_x[rep % 2]
            assert rx.tobytes() == sx[0].tobytes() and ix_ == sx[1]
            assert all((a == b).all() for a, b in zip(osp, sx[2][0])) and all((a == b).all() for a, b in zip(ofl, sx[2][1]))
            assert got[("v", rep)].tobytes() == serial_v[rep % 2].tobytes()
    finally:
        eng.close()
