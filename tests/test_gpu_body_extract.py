"""GPU: zke_extract_bodies (body_extract_kernel, csrc/bodyext.hip.h) against tests/body_model.py on infos and bytes, for both
positions of ZKE_BODYF_PART_KEEPS_EOL — the named edge list of tests/body_cases.py (base64 and quoted-printable at every step,
window, round and tile edge of the decode stream; selection, spans and Content-Transfer-Encoding spellings), the parse verdicts of
the MIME corpus against the verify path's own, batches around the wave count with all three encodings and failing e-mails, the
caller-sized buffer protocol, the asynchronous form through three slots, the seeded generator, and the C++ mirror.

The engine runs each named list ONCE per flag position (module-scoped fixture); the per-case tests read that answer."""
import ctypes as C
import glob
import json
import os
import subprocess

import numpy as np
import pytest

import body_cases as BC
import body_model as M
import zkemail_rs_amd as z
from zkemail_rs_amd import _abi as A
from zkemail_rs_amd import build
from zkemail_rs_amd.engine import _BodyBuffers

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
E_ARG, E_NOMEM = -1, -3
CASES = BC.all_cases()
NAMES = [n for n, _ in CASES]


def expected(raw, keep):
    """The model's answer in the shape of a BodyInfo: (status, detail) always; part, encoding, span and bytes where the e-mail got that far."""
    v = M.verdict(raw, keep)
    if v[0] == "ok":
        b = v[1]
        return (A.ZKE_OK, 0, b.part, b.encoding, b.src_off, b.src_len, b.data)
    if v[0] == "fail":
        lead = v[1] == "leading space"
        top = v[2] == 0
        return (A.ZKE_PARSE_FAIL, (A.D_HDR_LEADING_SPACE if lead else A.D_HDR_LONE_CR) if top else (A.D_SUBPART_LEADING_SPACE if lead else A.D_SUBPART_LONE_CR))
    if v[0] == "undecided":
        return (A.ZKE_UNSUPPORTED, v[1])
    return (A.ZKE_BODY_DECODE_FAIL, v[1], v[2], v[3], v[4], v[5], b"")


def check(got, raw, keep, what):
    want = expected(raw, keep)
    assert tuple(got)[:len(want)] == want, (what, keep, tuple(got)[:6], want[:6], got.body[:60], want[6][:60] if len(want) > 6 else None)
    if got.status != A.ZKE_OK:
        assert got.body == b""


@pytest.fixture(scope="module")
def answers(engine):
    return {keep: engine.extract_bodies([r for _, r in CASES], part_keeps_eol=keep) for keep in (False, True)}


@pytest.mark.parametrize("keep", [False, True], ids=["chop", "keeps_eol"])
@pytest.mark.parametrize("k", range(len(CASES)), ids=NAMES)
def test_named_case(answers, k, keep):
    check(answers[keep][k], CASES[k][1], keep, NAMES[k])


def test_worked_examples_and_statuses(answers):
    """The header's worked examples and the named details, spelled out (not through the model)."""
    by = dict(zip(NAMES, answers[False]))
    for k, (_, want) in enumerate(BC.QP_EXAMPLES):
        assert (by[f"qp_example_{k}"].status, by[f"qp_example_{k}"].body) == (A.ZKE_OK, want), k
    for name, detail in (("b64_vt_inside", A.D_BODY_B64_CHAR), ("b64_pad_in_the_middle", A.D_BODY_B64_CHAR), ("b64_missing_padding", A.D_BODY_B64_LENGTH),
                         ("b64_trailing_bits_two_pads", A.D_BODY_B64_TRAILING_BITS), ("b64_trailing_bits_one_pad", A.D_BODY_B64_TRAILING_BITS),
                         ("b64_bad_character_in_an_early_round", A.D_BODY_B64_CHAR), ("b64_trailing_bits_after_two_rounds", A.D_BODY_B64_TRAILING_BITS)):
        assert (by[name].status, by[name].detail, by[name].encoding) == (A.ZKE_BODY_DECODE_FAIL, detail, A.CTE_BASE64), name
    for name in ("cte_encoded_word", "cte_not_even_a_word", "cte_high_byte"):
        assert (by[name].status, by[name].detail) == (A.ZKE_UNSUPPORTED, A.D_U_BODY_CTE), name
    assert (by["b64_clean_0"].status, by["b64_clean_0"].body, by["b64_only_white_space"].body, by["b64_clean_8"].body) == (0, b"", b"", b"ABCDEF")
    assert by["sel_html_second_of_three"].part == 2 | A.BODY_PART_HTML and by["sel_html_second_of_three"].body == b"<b>hi</b>"
    assert by["sel_html_only_nested"].part == 1 and by["sel_html_only_nested"].body == b"inner preamble"
    assert dict(zip(NAMES, answers[True]))["sel_html_only_nested"].body == b"inner preamble\r\n"
    big = by["qp_lf_body_outgrows_the_email"]            # 300 lone LF: 299 CRLF, more bytes than the whole e-mail has
    assert big.status == 0 and big.body == b"\r\n" * 299 and len(big.body) > len(dict(CASES)["qp_lf_body_outgrows_the_email"])


def test_parse_verdicts_are_the_verify_paths(engine):
    """Every corpus_mime_* e-mail: where verify_email stops at the parse (header split, MIME walk), the extraction reports the same status
    and detail for the same bytes; where it does not, the extraction has no parse verdict either."""
    man = {c["eml"]: c for c in json.load(open(os.path.join(HERE, "golden", "ref_manifest.json")))["cases"]}
    paths = sorted(glob.glob(os.path.join(HERE, "golden", "ref_cases", "corpus_mime_*.eml")))
    assert len(paths) >= 10
    emails, raws = [], []
    for p in paths:
        c = man["ref_cases/" + os.path.basename(p)]
        raw = open(p, "rb").read()
        raws.append(raw)
        emails.append(A.Email(c["from_domain"], raw, A.PublicKey(bytes.fromhex(c["key_hex"]), c["key_type"])))
    rec = engine.verify_emails(emails)
    got = engine.extract_bodies(raws)
    parse_details = {A.D_HDR_LEADING_SPACE, A.D_HDR_LONE_CR, A.D_SUBPART_LEADING_SPACE, A.D_SUBPART_LONE_CR, A.D_U_TOO_MANY_HEADERS,
                     A.D_U_MIME_CTYPE, A.D_U_MIME_BOUNDARY, A.D_U_MIME_DEPTH}
    stopped = 0
    for p, r, g, raw in zip(paths, rec, got, raws):
        st, d = int(r["status"]), int(r["detail"])
        if st == A.ZKE_PARSE_FAIL or (st == A.ZKE_UNSUPPORTED and d in parse_details):
            assert (g.status, g.detail) == (st, d), os.path.basename(p)
            stopped += 1
        else:
            assert g.status != A.ZKE_PARSE_FAIL and not (g.status == A.ZKE_UNSUPPORTED and g.detail in parse_details), os.path.basename(p)
            check(g, raw, False, os.path.basename(p))
    assert stopped >= 3


def mixed(n, seed=0):
    """n e-mails that mix the three encodings, selection shapes and failing e-mails (named cases and generated ones in turn)."""
    gen = BC.generated(100 + seed, n)
    picks = [r for name, r in CASES if name.startswith(("sel_", "cte_", "fail_", "b64_clean_", "b64_trailing", "qp_example", "qp_lf", "qp_three", "u_"))]
    return [picks[(7 * i + seed) % len(picks)] if i % 2 else gen[i] for i in range(n)]


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batches_have_private_places(engine, n):
    raws = mixed(n, n)
    for keep in (False, True):
        got = engine.extract_bodies(raws, part_keeps_eol=keep)
        assert len(got) == n
        for i, (g, raw) in enumerate(zip(got, raws)):
            check(g, raw, keep, f"batch of {n}, e-mail {i}")
    if n == 65:
        kinds = {(g.status, g.encoding) for g in got}
        assert {(0, A.CTE_IDENTITY), (0, A.CTE_BASE64), (0, A.CTE_QP)} <= kinds and any(g.status for g in got)
    assert engine.extract_bodies([]) == []


def test_buffer_protocol(engine):
    raws = mixed(20, 5) + [dict(CASES)["qp_lf_lines_outgrow_the_email"]]
    exp = [expected(r, False) for r in raws]
    need = sum(len(x[6]) for x in exp if len(x) > 6)
    assert need > 0
    n = len(raws)
    b = _BodyBuffers(raws)
    b.c.infos_cap = n - 1
    assert engine.lib.zke_extract_bodies(engine.h, b.arr, b.n, 0, C.byref(b.c)) == E_NOMEM and (int(b.c.infos_need), int(b.c.bytes_need)) == (n, 0)
    for cap in (0, need - 1):
        b = _BodyBuffers(raws, cap)
        assert engine.lib.zke_extract_bodies(engine.h, b.arr, b.n, 0, C.byref(b.c)) == E_NOMEM, cap
        assert (int(b.c.infos_need), int(b.c.bytes_need)) == (n, need)
        off = 0
        for f, x in zip(b.infos, exp):                  # the infos are delivered all the same, body_off as it will be
            assert (int(f["status"]), int(f["detail"])) == x[:2]
            assert int(f["body_off"]) == off and int(f["body_len"]) == (len(x[6]) if len(x) > 6 else 0)
            off += int(f["body_len"])
    b = _BodyBuffers(raws, need)
    assert engine.lib.zke_extract_bodies(engine.h, b.arr, b.n, 0, C.byref(b.c)) == 0 and int(b.c.bytes_need) == need
    for g, raw in zip(b.result(), raws):
        check(g, raw, False, "exact buffer")
    assert engine.lib.zke_extract_bodies(engine.h, b.arr, b.n, 2, C.byref(b.c)) == E_ARG
    # the asynchronous form: the shortfall is reported by the wait
    b = _BodyBuffers(raws, need - 1)
    t = C.c_uint64()
    assert engine.lib.zke_extract_bodies_async(engine.h, b.arr, b.n, 0, C.byref(b.c), C.byref(t)) == 0
    assert engine.lib.zke_batch_wait(engine.h, t.value) == E_NOMEM and int(b.c.bytes_need) == need
    assert z.extract_email_body(dict(CASES)["sel_html_qp"], engine=engine) == "<p>café!</p>".encode()
    with pytest.raises(z.VerifyPanic) as e:
        z.extract_email_body(dict(CASES)["b64_missing_padding"], engine=engine)
    assert (e.value.status, e.value.detail) == (A.ZKE_BODY_DECODE_FAIL, A.D_BODY_B64_LENGTH) and "email.rs:17-21" in str(e.value)


def test_async_through_three_slots_equals_sync():
    eng = z.Engine(slots=3)
    batches = [mixed(40, s) for s in range(6)]
    for keep in (False, True):
        sync = [eng.extract_bodies(b, part_keeps_eol=keep) for b in batches]
        pend = [eng.extract_bodies_async(b, part_keeps_eol=keep) for b in batches]       # six batches in flight over three slots
        for (t, p), want in zip(pend, sync):
            eng.wait(t)
            assert p.result() == want
    for g, raw in zip(sync[0], batches[0]):
        check(g, raw, True, "slots")
    eng.close()


def test_second_call_of_the_same_shape_allocates_nothing():
    """Per-slot buffers come into being with the first call and only grow: device memory in use is the same before and after a second call."""
    hip = C.CDLL("libamdhip64.so")              # the runtime the engine's library is linked with: the same instance

    def free_bytes():
        free, total = C.c_size_t(), C.c_size_t()
        assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        return free.value

    eng = z.Engine(slots=1)
    raws = mixed(64, 9)
    first = eng.extract_bodies(raws)
    same = False
    for _ in range(5):            # (the figure is the device's, not the process's: another tenant's allocation may move it — not five times in a row)
        free0 = free_bytes()
        assert eng.extract_bodies(raws) == first and eng.extract_bodies(raws[:10]) == first[:10]
        same = free_bytes() == free0
        if same:
            break
    assert same
    eng.close()


@pytest.mark.parametrize("seed", [1, 2])
def test_seeded_fuzz(engine, seed):
    """512 generated e-mails in two batches: byte-identical to the model wherever it decides, ZKE_UNSUPPORTED exactly where it does not."""
    raws = BC.generated(seed, 256)
    for keep in (False, True):
        got = engine.extract_bodies(raws, part_keeps_eol=keep)
        undecided = 0
        for i, (g, raw) in enumerate(zip(got, raws)):
            check(g, raw, keep, f"seed {seed} e-mail {i}")
            undecided += g.status == A.ZKE_UNSUPPORTED
        assert 0 < undecided <= len(raws) // 10


def test_cpp_mirror(tmp_path):
    exe = build.build_cpp_body()
    names = ["sel_html_second_of_three", "sel_html_qp", "cte_base64_broken_in_the_html_part", "fail_child_leading_space", "b64_missing_padding", "cte_encoded_word"]
    paths = []
    for nm in names:
        (tmp_path / (nm + ".eml")).write_bytes(dict(CASES)[nm])
        paths.append(str(tmp_path / (nm + ".eml")))
    r = subprocess.run([exe, "0"] + paths, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 2 * len(names)
    for nm, info, single in zip(names, lines[:len(names)], lines[len(names):]):
        want = expected(dict(CASES)[nm], False)
        f = info.split(" ")
        assert f[0] == "INFO" and tuple(int(x) for x in f[1:3]) == want[:2], (nm, info)
        if len(want) > 6:
            assert tuple(int(x) for x in f[3:7]) == want[2:6] and bytes.fromhex(f[7] if len(f) > 7 else "") == want[6], (nm, info)
        if want[0] == A.ZKE_OK:
            assert single == "BODY " + want[6].hex(), (nm, single)
        else:
            site = "email.rs:26" if want[0] == A.ZKE_PARSE_FAIL else "email.rs:21" if nm == "cte_base64_broken_in_the_html_part" else \
                "email.rs:17" if nm == "b64_missing_padding" else "email.rs:21"
            assert single.startswith("PANIC %d %d " % want[:2]) and site in single, (nm, single)
