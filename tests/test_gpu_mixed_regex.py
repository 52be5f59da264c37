"""GPU parity (-m gpu): zke_verify_emails_mixed — `&[EmailWithRegex]` whose values carry different regex configs, and e-mails
without one, in ONE batch — against the oracle run per config (tests/mixed_cases.py: group, run as today, scatter back), field by
field.  The cases about a kernel run under dfa_mapping 1 (the lane-mapped launch) and 2 (the wave-mapped one)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mixed_cases as mc
import zkemail_rs_amd as z
from zkemail_rs_amd import _abi as A
from zkemail_rs_amd import build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAPPINGS = [1, 2]


@pytest.fixture(scope="module")
def engines():
    return {1: z.Engine(dfa_mapping=1), 2: z.Engine(dfa_mapping=2)}


def run_case(eng, oracle, inputs, keys, ctx, regex_failures=False, all_fail=()):
    exp = mc.expectation(oracle, inputs, keys)
    mc.check_not_vacuous(exp, keys, regex_failures, all_fail)
    got = eng.verify_emails_mixed(inputs)
    mc.assert_equal(got, exp, ctx)
    return got, exp


@pytest.mark.parametrize("mapping", MAPPINGS)
def test_sizes_and_orders(engines, oracle, mapping):
    """n = 1; three configs interleaved i % 3, then the same list sorted by config, then reversed."""
    eng = engines[mapping]
    for name in ("B", None, "ZERO"):
        one = [mc.make_input(0, name)]
        exp = mc.expectation(oracle, one, [name])
        assert int(exp[0]["status"]) == A.ZKE_OK
        mc.assert_equal(eng.verify_emails_mixed(one), exp, f"n=1 {name}")
    names = ["A", "B", "C"]
    keys = [names[i % 3] for i in range(48)]
    inputs = mc.workload(keys)
    got, exp = run_case(eng, oracle, inputs, keys, "interleaved", regex_failures=True)
    order = sorted(range(48), key=lambda i: keys[i])
    for tag, perm in (("sorted", order), ("reversed", order[::-1])):
        g2 = eng.verify_emails_mixed([inputs[i] for i in perm])
        mc.assert_equal(g2, exp[perm], tag)


@pytest.mark.parametrize("mapping", MAPPINGS)
def test_tile_edges(engines, oracle, mapping):
    """Configs of exactly 256 and of 257 e-mails (the lane launch's block), of 4 and of 5 (the wave launch's), and between two
    populated configs one that no e-mail names: it has segments and no blocks."""
    eng = engines[mapping]
    keys = ["A"] * 256 + ["D"] * 4 + ["B"] * 257 + ["C"] * 5
    inputs = mc.workload(keys)
    exp = mc.expectation(oracle, inputs, keys)
    mc.check_not_vacuous(exp, keys, True)
    # the empty config sits between "A" and "D": its id list is registered, no e-mail refers to it
    lists = eng.pack_mixed(inputs)
    empty = mc.make_input(0, "NINE")
    ids = ([eng.dfa_register(p.verify_re.fwd, p.verify_re.bwd) for p in empty.regex_info.header_parts],
           [eng.dfa_register(p.verify_re.fwd, p.verify_re.bwd) for p in empty.regex_info.body_parts])
    assert len(lists.configs) == 4
    configs = [lists.configs[0], ids] + lists.configs[1:]
    config_of = [c if c == 0 else c + 1 for c in lists.config_of[:len(keys)]]
    caps = [[list(p.captures or []) for p in (i.regex_info.header_parts or []) + (i.regex_info.body_parts or [])] for i in inputs]
    ml = A.MixedLists(configs, config_of, caps)
    refs = A.EmailRefs([i.email for i in inputs])
    got = np.zeros(len(inputs), dtype=A.RESULT_DTYPE)
    rc = eng.lib.zke_verify_emails_mixed(eng.h, refs.arr, refs.n, C.byref(ml.c), got.ctypes.data)
    assert rc == 0, eng.lib.zke_last_error(eng.h)
    mc.assert_equal(got, exp, "tile edges")


@pytest.mark.parametrize("mapping", MAPPINGS)
def test_shapes_of_p(engines, oracle, mapping):
    """One part beside nine (more than a single-config launch holds); one pair as a header part in one config and a body part in
    another; a zero-part config beside e-mails without a config, over e-mails whose first signature is not the verified one."""
    eng = engines[mapping]
    keys = [("ONE", "NINE")[i % 2] for i in range(24)]
    run_case(eng, oracle, mc.workload(keys), keys, "1 beside 9", regex_failures=True)
    # pool e-mails 2, 10, 18 carry the ORDER marker in their Subject too
    keys = ["ORDER_IN_HEADER", "D"] * 12
    inputs = mc.workload(keys, start=2, spoil=False)
    got, exp = run_case(eng, oracle, inputs, keys, "header and body")
    lists = eng.pack_mixed(inputs)
    assert lists.configs[0][0] == lists.configs[1][1] and len(lists.configs[0][0]) == 1       # the same id on both sides
    assert {int(exp[i]["status"]) for i in range(0, 24, 2)} >= {A.ZKE_OK, A.ZKE_HEADER_REGEX_FAIL}
    # zero parts is not "no config": canonicalize_signed_email still runs (circuits.rs:34-35) and can fail
    two = mc.two_signature_mails()
    plain = [mc.pool()[i].email for i in (0, 1, 5)]
    inputs = [A.EmailWithRegex(e, A.RegexInfo(None, None)) for e in two + plain] + two + plain
    keys = ["ZERO"] * 5 + [None] * 5
    exp = mc.expectation(oracle, inputs, keys)
    assert int(exp[6]["status"]) == A.ZKE_OK and int(exp[1]["status"]) == A.ZKE_CANON_FAIL      # the same e-mail, with and without
    assert int(exp[0]["status"]) == A.ZKE_OK and int(exp[4]["status"]) == int(exp[9]["status"]) == A.ZKE_DKIM_NOT_PASS
    mc.assert_equal(eng.verify_emails_mixed(inputs), exp, "zero parts beside none")


@pytest.mark.parametrize("mapping", MAPPINGS)
def test_status_paths_per_config(engines, oracle, mapping):
    """A failing first part hides a later one; a capture is missing; the signature is bad; external_input_null; a junk pair fails
    the e-mails of its own config only."""
    eng = engines[mapping]
    keys = ["THREE"] * 4 + ["A"] * 6 + ["B"] * 6
    inputs = mc.workload(keys, spoil=False)
    inputs[1].regex_info.header_parts[0].captures = ["not in the subject"]            # THREE: part 0 fails and hides ...
    inputs[1].regex_info.body_parts[0].captures = ["99999999x"]                       # ... part 2, which would fail too
    inputs[2].regex_info.body_parts[0].captures = ["99999999x"]                       # (alone it is reported)
    inputs[4].regex_info.header_parts[1].captures = ["nobody"]                        # A: capture missing in its second part
    assert mc.pool()[5].kind == "badsig"                                              # A: inputs[5] has a bad signature
    inputs[8] = A.EmailWithRegex(A.Email("example.com", inputs[8].email.raw_email, inputs[8].email.public_key,
                                         [A.ExternalInput("n", None)]), inputs[8].regex_info)
    junk = A.RegexInfo([A.CompiledRegex(A.DFA(b"junk", b"junk"), ["x"])], [A.CompiledRegex(mc.dfa_of(mc.B_ORDER[0]), [])])
    inputs += [A.EmailWithRegex(mc.pool()[i].email, junk) for i in (0, 1, 5)]
    keys += ["JUNK"] * 3
    exp = mc.expectation(oracle, inputs, keys)
    mc.check_not_vacuous(exp, keys, False, all_fail=("JUNK",))
    st = [int(x) for x in exp["status"]]
    assert st[0] == A.ZKE_OK
    assert st[1] == A.ZKE_HEADER_REGEX_FAIL and int(exp[1]["regex_part"]) == 0 and int(exp[1]["detail"]) == A.D_RE_CAPTURE_MISSING
    assert st[2] == A.ZKE_BODY_REGEX_FAIL and int(exp[2]["regex_part"]) == 2
    assert st[4] == A.ZKE_HEADER_REGEX_FAIL and int(exp[4]["regex_part"]) == 1
    assert st[5] == A.ZKE_DKIM_NOT_PASS and st[8] == A.ZKE_EXTERNAL_INPUT_NULL
    assert st[16:] == [A.ZKE_DFA_DECODE_FAIL, A.ZKE_DFA_DECODE_FAIL, A.ZKE_DKIM_NOT_PASS]
    assert A.ZKE_OK in st[4:10] and A.ZKE_OK in st[10:16]
    mc.assert_equal(eng.verify_emails_mixed(inputs), exp, "status paths")


@pytest.mark.parametrize("mapping", MAPPINGS)
def test_large_tables_share_a_launch(engines, oracle, mapping):
    """A pair compiled in Unicode mode whose two blobs exceed 160 KiB — more than a CU has of LDS: its segment walks the tables from
    HBM — in one launch with pairs of a few KB, which are staged in LDS."""
    eng = engines[mapping]
    big = mc.dfa_of(mc.UNI_ORDER, True)
    assert len(big.fwd) + len(big.bwd) > 160 * 1024
    small = mc.dfa_of(mc.B_ORDER[0])
    assert len(small.fwd) + len(small.bwd) < 32 * 1024
    inputs, keys = [], []
    for i in range(12):
        m = mc.pool()[i]
        order = m.clean_body[m.clean_body.find(b"ZKE-ORDER-") + 10:][:8].decode()
        d = big if i % 2 else small
        inputs.append(A.EmailWithRegex(m.email, A.RegexInfo(None, [A.CompiledRegex(d, [order if i != 3 else "00000000x"])])))
        keys.append("BIG" if i % 2 else "SMALL")
    got, exp = run_case(eng, oracle, inputs, keys, "large tables")
    assert int(exp[3]["status"]) == A.ZKE_BODY_REGEX_FAIL


@pytest.mark.parametrize("mapping", MAPPINGS)
def test_capture_counts_differ_per_part(engines, oracle, mapping):
    """0, 1, 2 and 3 capture strings per part, different for every e-mail: a wrong job index reads a neighbour's strings."""
    eng = engines[mapping]
    keys = [("A", "B", None, "C")[i % 4] for i in range(32)]
    inputs = mc.workload(keys, spoil=False)
    rng = np.random.default_rng(7)
    bad = set()
    for k, inp in enumerate(inputs):
        if keys[k] is None:
            continue
        for p in (inp.regex_info.header_parts or []) + (inp.regex_info.body_parts or []):
            good = p.captures[0]
            cnt = int(rng.integers(0, 4))
            p.captures = [good[:1 + j] for j in range(cnt)]            # prefixes of the real capture: contained in the match
        if k % 8 == 5:                                                 # ... and one string that belongs to nobody
            p.captures = list(p.captures) + ["zz-not-there"]
            bad.add(k)
    exp = mc.expectation(oracle, inputs, keys)
    mc.check_not_vacuous(exp, keys, False)
    for k in bad:
        if mc.pool()[k % mc.POOL_N].kind == "plain":
            assert int(exp[k]["detail"]) == A.D_RE_CAPTURE_MISSING
    mc.assert_equal(eng.verify_emails_mixed(inputs), exp, "capture counts")
    lists = eng.pack_mixed(inputs)
    assert len(set(np.diff(lists.cap_off.astype(np.int64)))) >= 3


def test_call_failures(engine, oracle):
    """ZKE_E_ARG with a message, before anything is staged: a config_of that names no config, too many configs, too many parts, a
    null list with a count, capture offsets that decrease; the engine verifies the next batch as if nothing had happened."""
    inputs = mc.workload(["A", "B", None, "A"], spoil=False)
    refs = A.EmailRefs([i if isinstance(i, A.Email) else i.email for i in inputs])
    out = np.zeros(refs.n, dtype=A.RESULT_DTYPE)

    def call(ml):
        rc = engine.lib.zke_verify_emails_mixed(engine.h, refs.arr, refs.n, C.byref(ml.c), out.ctypes.data)
        return rc, engine.lib.zke_last_error(engine.h).decode()

    ml = engine.pack_mixed(inputs)
    ml.config_of[1] = 2                                   # two configs: 2 names none, and is not ZKE_CONFIG_NONE
    rc, msg = call(ml)
    assert rc == -1 and "config_of" in msg
    ml = engine.pack_mixed(inputs)
    ml.c.n_configs = A.MIXED_MAX_CONFIGS + 1
    rc, msg = call(ml)
    assert rc == -1 and "ZKE_MIXED_MAX_CONFIGS" in msg
    ml = engine.pack_mixed(inputs)
    ml.arr[0].n_header_parts = A.MIXED_MAX_PARTS + 1
    rc, msg = call(ml)
    assert rc == -1 and "ZKE_MIXED_MAX_PARTS" in msg
    ml = engine.pack_mixed(inputs)
    ml.arr[1].body_part_ids = None
    rc, msg = call(ml)
    assert rc == -1 and "null" in msg
    ml = engine.pack_mixed(inputs)
    ml.c.config_of = None
    rc, msg = call(ml)
    assert rc == -1 and "null" in msg
    ml = engine.pack_mixed(inputs)
    assert ml.cap_off[2] > 0
    ml.cap_off[3] = ml.cap_off[2] - 1
    rc, msg = call(ml)
    assert rc == -1 and "non-decreasing" in msg
    keys = ["A", "B", None, "A"]
    exp = mc.expectation(oracle, inputs, keys)
    mc.check_not_vacuous(exp, keys, False)
    mc.assert_equal(engine.verify_emails_mixed(inputs), exp, "after the refused calls")


def test_three_slots_alternating_entries(oracle):
    """The asynchronous entry through 3 slots: mixed batches, single-config zke_verify_emails_with_regex batches and zke_verify_emails
    batches in turn on one engine, waited for at the end; every batch equals its serial run and the oracle."""
    eng = z.Engine(slots=3)
    batches = []
    for r in range(3):
        keys = [("A", "B", None, "D")[(i + r) % 4] for i in range(20 + r)]
        batches.append(("mixed", mc.workload(keys, start=r), keys))
        keys = ["B"] * (9 + r)
        batches.append(("regex", mc.workload(keys, start=3 * r), keys))
        keys = [None] * (7 + r)
        batches.append(("plain", mc.workload(keys, start=5 * r), keys))
    serial = []
    for kind, inputs, keys in batches:
        exp = mc.expectation(oracle, inputs, keys)
        if kind != "plain":
            mc.check_not_vacuous(exp, keys, False)
        serial.append(exp)
    pending, keep = [], []
    lib = eng.lib
    for kind, inputs, keys in batches:
        if kind == "mixed":
            pending.append(eng.verify_emails_mixed_async(inputs))
        elif kind == "plain":
            pending.append(eng.verify_emails_async(A.EmailRefs(inputs)))
        else:
            p = eng.pack_with_regex(inputs)
            refs = A.EmailRefs([i.email for i in inputs])
            lists = A.zke_regex_lists()
            lists.n_header_parts, lists.n_body_parts = p.nh, p.nb
            lists.header_part_ids, lists.body_part_ids = p.hdr_ids.ctypes.data, p.body_ids.ctypes.data
            lists.cap_off, lists.cap_str_off, lists.cap_blob = p.cap_off.ctypes.data, p.cap_str_off.ctypes.data, p.cap_blob.ctypes.data
            out = np.zeros(refs.n, dtype=A.RESULT_DTYPE)
            t = C.c_uint64()
            assert lib.zke_verify_emails_with_regex_async(eng.h, refs.arr, refs.n, C.byref(lists), out.ctypes.data, C.byref(t)) == 0
            keep.append((p, refs, lists))
            pending.append((t.value, out))
    for t, _ in pending:
        eng.wait(t)
    for (kind, inputs, keys), (_, got), exp in zip(batches, pending, serial):
        mc.assert_equal(got, exp, f"slots: {kind} n={len(inputs)}")
    eng.close()


def test_default_mapping_above_1024(engine, oracle):
    """Without a forced mapping a batch of more than 1 024 e-mails sends header parts to the lane launch and body parts to the wave
    launch: both launches in one batch, and e-mails without a config among them."""
    keys = [("B", "C", None, "A", "D")[i % 5] for i in range(1100)]
    inputs = mc.workload(keys)
    run_case(engine, oracle, inputs, keys, "default mapping", regex_failures=True)


def test_cpp_mirror(oracle):
    """zkemail::verify_emails_mixed of include/zkemail_core.hpp (tests/cpp/mixed_test.cpp): the program verifies the .eml files it
    is given, the first half with one config, the second half with another, the last one without, and prints the records."""
    exe = build.build_cpp_mixed()
    import tempfile
    inputs = mc.workload(["A"] * 3 + ["D"] * 3 + [None], spoil=False)
    keys = ["A"] * 3 + ["D"] * 3 + [None]
    exp = mc.expectation(oracle, inputs, keys)
    mc.check_not_vacuous(exp, keys, False)
    with tempfile.TemporaryDirectory() as tmp:
        args = []
        for k, inp in enumerate(inputs):
            em = inp if isinstance(inp, A.Email) else inp.email
            for ext, data in (("eml", em.raw_email), ("key", em.public_key.key)):
                with open(os.path.join(tmp, f"m{k}.{ext}"), "wb") as f:
                    f.write(data)
            args.append(os.path.join(tmp, f"m{k}"))
        pats = [tmp + "/a0.dfa", tmp + "/a1.dfa", tmp + "/d0.dfa"]
        for path, (pat, _) in zip(pats, mc.CONFIGS["A"][0] + mc.CONFIGS["D"][1]):
            d = mc.dfa_of(pat)
            open(path + ".fwd", "wb").write(d.fwd)
            open(path + ".bwd", "wb").write(d.bwd)
        caps = os.path.join(tmp, "caps.txt")
        with open(caps, "w") as f:
            for inp in inputs[:6]:
                for p in (inp.regex_info.header_parts or []) + (inp.regex_info.body_parts or []):
                    f.write("\t".join(p.captures or []) + "\n")
        r = subprocess.run([exe, caps] + pats + ["--"] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("record")]
    assert len(lines) == len(inputs)
    for i, ln in enumerate(lines):
        want = [int(exp[i][f]) for f in ("status", "detail", "regex_part", "match_count", "match_start", "match_end")]
        assert [int(x) for x in ln[2:8]] == want, (i, ln, want)
        assert ln[8] == bytes(exp[i]["header_hash"]).hex()
