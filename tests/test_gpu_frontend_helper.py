"""GPU parity (-m gpu) for the two-wave round-0 front end (csrc/parse.hip.h, parse_kernel<true>): the helper wave canonicalises
the body while the front-end wave writes the header-hash preimage.  Every record must be the oracle's, field for field, through
the hand-off (body geometry of the canonicaliser's thresholds), on every exit of the front-end wave with a live helper beside
it, on the paths where the front-end wave canonicalises by itself after all, and across repeated runs of both entry points."""
import hashlib
import os

import numpy as np
import pytest

import cases
import synth
from synth import SignSpec, sign_email
from zkemail_rs_amd import _abi as A
from test_gpu_verify import assert_records_equal, run_both

pytestmark = pytest.mark.gpu


def _engine_with(knob):
    """An engine created with ZKE_FRONT_HELPER = knob in the environment (None: unset); the variable is read at zke_engine_create."""
    import zkemail_rs_amd as z
    old = os.environ.pop("ZKE_FRONT_HELPER", None)
    if knob is not None:
        os.environ["ZKE_FRONT_HELPER"] = knob
    try:
        return z.Engine()
    finally:
        os.environ.pop("ZKE_FRONT_HELPER", None)
        if old is not None:
            os.environ["ZKE_FRONT_HELPER"] = old


@pytest.fixture(scope="module")
def engine():
    """An engine that takes the two-wave front end for every batch, and says so (zke_engine_front_helper); unset, the stage plan
    takes it for batches of up to 1 024 e-mails where the ring is taken (at most four batches in flight at once)."""
    eng, off, plain = _engine_with("1"), _engine_with("0"), _engine_with(None)
    assert all(eng.front_helper(n) for n in (1, 2, 65, 340, 1024, 1025, 8192))
    assert not any(off.front_helper(n) for n in (1, 1024, 8192))
    assert not plain.front_helper(1025) and plain.front_helper(1) == plain.front_helper(1024)
    off.close()
    plain.close()
    yield eng
    eng.close()


# window edge, last-group clean-prefix threshold, the ring's refill, the LDS flush threshold, one body the helper is still busy
# with long after the preimage is written
LENGTHS = [0, 1, 2, 255, 256, 257, 320, 321, 2047, 2048, 2049, 3503, 3504, 3505, 3506, 4096, 65536]


def clean_body(n: int, seed: int) -> bytes:
    if n < 3:
        return b"ab"[:n]
    return synth.ascii_body(np.random.default_rng(seed), n)


DIRTY_UNIT = b"ab \t cd\t\tef  \r\n"          # 15 bytes: no 256-byte window of its repetitions is clean


def dirty_body(n: int, ending: str) -> bytes:
    """n bytes in which every window has TAB and SP runs and trailing WSP; `ending`: "cut" (no final CRLF), "wsp" (the body
    ends in a WSP run) or "crlfs" (many trailing empty lines)."""
    b = bytearray((DIRTY_UNIT * (n // len(DIRTY_UNIT) + 1))[:n])
    if ending == "wsp" and n >= 2:
        b[-2:] = b" \t"
    elif ending == "crlfs":
        k = min(45, n // 2)
        if k:
            b[n - 2 * k:] = b"\r\n" * k
    if n and b[-1] == 0x0D:                    # no lone CR at the very end (the Python signer splits lines at CRLF)
        b[-1] = ord("x")
    return bytes(b)


def geometry_emails():
    k0, k1 = synth.keys_of(2048, 2)
    out = []

    def add(name, body, spec, key):
        raw, it = sign_email(cases._hdrs(len(out)), body, key, spec)
        out.append((name, A.Email("example.com", raw, A.PublicKey(key.pkcs1_der)), it))

    for j, n in enumerate(LENGTHS):
        key = (k0, k1)[j % 2]
        cb = clean_body(n, 700 + j)
        bodies = [("clean", cb)] + [(f"dirty_{e}", dirty_body(n, e)) for e in ("cut", "wsp", "crlfs")]
        for bn, body in bodies:
            for bc in ("relaxed", "simple"):
                add(f"{bn}_{bc}_{n}", body, SignSpec(body_canon=bc), key)
        # l= shorter than, equal to and longer than the canonical length
        for bn, body in bodies:
            for bc in ("relaxed", "simple"):
                full = len(synth.relaxed_body(body) if bc == "relaxed" else synth.simple_body(body))
                for ln, L in (("short", full // 2), ("equal", full), ("long", full + 7)):
                    add(f"{bn}_{bc}_{n}_l_{ln}", body, SignSpec(body_canon=bc, length=L), key)
    return out


def check_against_oracle(got, exp, d1, d2, names, ctx):
    assert_records_equal(got, exp, names, ctx)
    for i in range(len(exp)):
        bl = int(d2.full_len[i])
        assert int(d1.full_len[i]) == bl, (ctx, names[i])
        assert bytes(d1.canon_body[i, :bl]) == bytes(d2.canon_body[i, :bl]), (ctx, names[i])
        hl = int(exp[i]["canon_header_len"])
        assert bytes(d1.canon_header[i, :hl]) == bytes(d2.canon_header[i, :hl]), (ctx, names[i])


def test_canonicaliser_geometry_through_the_hand_off(engine, oracle):
    """Body lengths at every threshold of the relaxed canonicaliser, clean and with every window dirty, relaxed and simple, with
    l= below, at and beyond the canonical length: records, canonical bodies and preimages are the oracle's, and what the Python
    signer signed verifies."""
    cs = geometry_emails()
    names = [c[0] for c in cs]
    got, exp, d1, d2 = run_both(engine, oracle, [c[1] for c in cs])
    check_against_oracle(got, exp, d1, d2, names, "geometry")
    n_ok = 0
    for i, (name, _, it) in enumerate(cs):
        if int(exp[i]["status"]) != A.ZKE_OK:
            continue
        n_ok += 1
        assert bytes(got[i]["body_hash"]) == it["body_hash"] and bytes(got[i]["header_hash"]) == it["header_hash"], name
        assert int(got[i]["canon_body_len"]) == it["hashed_body_len"], name
    # the clean bodies all verify; of the dirty ones, those whose end cfdkim canonicalises as RFC 6376 does
    not_ok = [(n, int(exp[i]["status"]), int(exp[i]["detail"])) for i, n in enumerate(names) if n.startswith("clean") and int(exp[i]["status"]) != A.ZKE_OK]
    assert not not_ok, not_ok[:5]
    assert n_ok > len(cs) // 2


BAD_KINDS = ("too_many_headers", "mime_subpart", "key_der_garbage", "key_type", "no_signature", "other_domain", "bad_c", "bad_l",
             "bad_a", "tag_syntax", "ed25519")


def exit_emails():
    """{kind: (email, status, detail)} for every way the front-end wave ends early, and four good e-mails."""
    k0 = cases.K()
    hs, body = cases._hdrs(8), cases._body(300, 12)
    mk = cases.mk
    mp = b'multipart/alternative; boundary="=_b0"'
    mime_bad = (b"preamble\r\n--=_b0\r\n Content-Type: text/plain; charset=utf-8\r\n\r\nplain text\r\n--=_b0--\r\n")
    bad = {
        "too_many_headers": mk("x", [(b"X-Filler-%d" % i, b"v") for i in range(260)] + cases._hdrs(30), cases._body(200, 30), k0,
                               status=A.ZKE_UNSUPPORTED, detail=A.D_U_TOO_MANY_HEADERS),
        "mime_subpart": mk("x", cases._with_ctype(cases._hdrs(11), mp), mime_bad, k0, status=A.ZKE_PARSE_FAIL, detail=A.D_SUBPART_LEADING_SPACE),
        "key_der_garbage": mk("x", hs, body, k0, pubkey=b"\x30\x03\x02\x01", status=A.ZKE_KEY_DECODE_FAIL, detail=A.D_KEY_DER),
        "key_type": mk("x", hs, body, k0, key_type="dsa", status=A.ZKE_KEY_DECODE_FAIL, detail=A.D_KEY_TYPE),
        "no_signature": mk("x", hs, body, k0, mutate=lambda r: r[r.find(b"Received:"):], status=A.ZKE_DKIM_NOT_PASS, detail=A.D_NEUTRAL),
        "other_domain": mk("x", hs, body, k0, from_domain="other.org", status=A.ZKE_DKIM_NOT_PASS, detail=A.D_NEUTRAL),
        "bad_c": mk("x", hs, body, k0, SignSpec(c_tag="nofws/simple"), status=A.ZKE_DKIM_NOT_PASS, detail=A.D_BAD_CANON),
        "bad_l": mk("x", hs, body, k0, SignSpec(extra_tags="l=12x; "), status=A.ZKE_DKIM_NOT_PASS, detail=A.D_BAD_LENGTH),
        "bad_a": mk("x", hs, body, k0, SignSpec(algo="rsa-md5"), status=A.ZKE_DKIM_NOT_PASS, detail=A.D_BAD_ALGO),
        "tag_syntax": mk("x", hs, body, k0, mutate=lambda r: r.replace(b"DKIM-Signature: v=1;", b"DKIM-Signature: =1;", 1),
                         status=A.ZKE_DKIM_NOT_PASS, detail=A.D_SIG_SYNTAX),
        "ed25519": mk("x", hs, body, cases.ED()[0], key_type="ed25519"),
    }
    assert set(bad) == set(BAD_KINDS)
    good = [mk("g", cases._hdrs(60 + j), cases._body(n, 60 + j), k0, SignSpec(header_canon=hc, body_canon=bc))
            for j, (n, hc, bc) in enumerate(((300, "relaxed", "relaxed"), (5000, "relaxed", "relaxed"), (700, "simple", "simple"), (2600, "relaxed", "simple")))]
    return bad, good


def test_every_exit_of_the_front_end_wave_beside_a_live_helper(engine, oracle):
    """65 e-mails: good ones interleaved with each early exit of the front-end wave (the helper of such an e-mail is released
    by the kernel's tail).  The call returns and all 65 records equal the oracle's; then the same with n = 1 and n = 2."""
    bad, good = exit_emails()
    batch, names = [], []
    for k in range(65):
        if k % 2 == 1:
            kind = BAD_KINDS[(k // 2) % len(BAD_KINDS)]
            batch.append(bad[kind]); names.append(kind)
        else:
            batch.append(good[(k // 2) % len(good)]); names.append("good")
    assert len(batch) == 65 and names[64] == "good" and set(names) == set(BAD_KINDS) | {"good"}
    got, exp, d1, d2 = run_both(engine, oracle, [c.email for c in batch])
    check_against_oracle(got, exp, d1, d2, names, "exits")
    for i, c in enumerate(batch):                       # and both equal the expectation written down with the case
        assert int(got[i]["status"]) == c.status, names[i]
        if c.detail is not None:
            assert int(got[i]["detail"]) == c.detail, names[i]
    # n = 1: every kind alone; n = 2: beside a good e-mail, in both orders
    for kind in BAD_KINDS:
        for group in ([bad[kind]], [good[0], bad[kind]], [bad[kind], good[1]]):
            g, x, e1, e2 = run_both(engine, oracle, [c.email for c in group])
            check_against_oracle(g, x, e1, e2, [kind] * len(group), f"exits n={len(group)} {kind}")
            for i, c in enumerate(group):
                assert int(g[i]["status"]) == c.status, (kind, len(group), i)
    g, x, e1, e2 = run_both(engine, oracle, [good[2].email])
    check_against_oracle(g, x, e1, e2, ["good"], "exits n=1 good")
    assert int(g[0]["status"]) == A.ZKE_OK


def _sig_of(raw: bytes, first_name: bytes) -> bytes:
    return raw[:raw.find(first_name)]


def overflow_emails():
    """E-mails whose FIRST same-domain signature overflows the preimage's scratch slot: simple header canonicalisation, h= naming
    dkim-signature twice (both signature headers enter the preimage, then the signature itself once more), the header inflated by
    folding white space — which counts neither for ZKE_MAX_TAGBUF nor under relaxed canonicalisation.  The first signature is made
    over another body, so the reference fails it on the body hash and goes on to the second as well.
    -> (a) second signature with the OTHER body canonicalisation, (b) the same canonicalisation and a different l=,
       (w) the first signature alone: the witness that it overflows (the device reports it, the reference does not know the limit)"""
    k0 = cases.K()
    hs = [(b"From", b"a@example.com"), (b"To", b"b@example.net"), (b"Subject", b"overflow")]
    body = dirty_body(2600, "crlfs")
    pad = "z=pad;" + " " * 9000 + " "
    first = hs[0][0] + b":"
    out = {}
    for name, spec1, spec2 in (("a", SignSpec(body_canon="simple"), SignSpec(body_canon="relaxed")),
                               ("b", SignSpec(body_canon="relaxed", length=40), SignSpec(body_canon="relaxed", length=1000))):
        big = SignSpec(selector="big", header_canon="simple", body_canon=spec1.body_canon, length=spec1.length, extra_tags=pad,
                       signed=("from", "dkim-signature", "dkim-signature"))
        raw1, _ = sign_email(hs, cases._body(100, 5), k0, big)
        raw2, it = sign_email(hs, body, k0, spec2)
        out[name] = (A.Email("example.com", _sig_of(raw1, first) + raw2, A.PublicKey(k0.pkcs1_der)), it)
        if name == "a":
            out["w"] = (A.Email("example.com", _sig_of(raw1, first) + raw2[len(_sig_of(raw2, first)):], A.PublicKey(k0.pkcs1_der)), None)
    return out


def test_fallback_paths(engine, oracle):
    """The front-end wave canonicalises by itself (a) when the posted candidate's preimage overflowed and the next signature has
    the other body canonicalisation, (b) the same canonicalisation and another l=, (c) when the excised header was written to
    region B (a short b= value that occurs twice: no post); (d) later signature rounds run the one-wave path in the verdict launch."""
    ov = overflow_emails()
    # (w) the first signature does overflow on the device
    gw = engine.verify_batch(A.PackedBatch([ov["w"][0]]))
    assert (int(gw[0]["status"]), int(gw[0]["detail"])) == (A.ZKE_UNSUPPORTED, A.D_U_PREIMAGE_OVERFLOW)
    # (c) the shape of test_repeated_b_value_is_removed_everywhere, over a body worth canonicalising
    k0 = cases.K()
    raw, _ = sign_email(cases._hdrs(7), dirty_body(3505, "wsp"), k0, SignSpec(extra_tags="t=1790000000; ", fold_sig=False))
    i = raw.find(b" b=") + 3
    j = raw.find(b"\r\n", i)
    bval = raw[i:j]
    rep = [raw.replace(b"v=1;", b"v=1; z=" + bval + b";", 1), raw[:i] + b"AA" + raw[j:], raw[:i] + b"s" + raw[j:]]
    # (d) failing candidates first, the good signature in a later round: relaxed and simple bodies
    multi = [cases.multi_signature_case(1, body=dirty_body(2049, "crlfs")),
             cases.multi_signature_case(2, body=clean_body(3504, 3), spec=SignSpec(body_canon="simple")),
             cases.multi_signature_case(1, body=dirty_body(4096, "crlfs"), spec=SignSpec(length=100))]
    emails = [ov["a"][0], ov["b"][0]] + [A.Email("example.com", m, A.PublicKey(k0.pkcs1_der)) for m in rep] + [c.email for c in multi]
    names = ["overflow_other_canon", "overflow_other_l", "b_twice_full", "b_twice_AA", "b_twice_s", "round_1", "round_2_simple", "round_1_l"]
    got, exp, d1, d2 = run_both(engine, oracle, emails)
    check_against_oracle(got, exp, d1, d2, names, "fallback")
    for k, key in enumerate(("a", "b")):
        it = ov[key][1]
        assert int(got[k]["status"]) == A.ZKE_OK and int(got[k]["sig_index"]) == 1, names[k]
        assert bytes(got[k]["body_hash"]) == it["body_hash"] and bytes(got[k]["header_hash"]) == it["header_hash"], names[k]
    assert [int(got[k]["status"]) for k in (5, 6, 7)] == [A.ZKE_OK] * 3 and [int(got[k]["sig_index"]) for k in (5, 6, 7)] == [1, 2, 1]
    for k in (2, 3, 4):
        assert int(exp[k]["canon_header_len"]) > 0


def test_side_outputs_are_the_same_on_every_run():
    """One batch (geometry, exits and fallbacks mixed) twice through the device entry and once through the host entry: identical
    records; body hash and header hash equal hashlib over the oracle's canonical forms.  In a subprocess so that torch, which owns
    the device buffers, initialises HIP before the engine does."""
    import subprocess, sys, textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent(f"""
        import sys
        sys.path.insert(0, {root!r}); sys.path.insert(0, {os.path.join(root, 'tests')!r})
        import hashlib
        import numpy as np, torch
        torch.zeros(1, device="cuda")
        import bench, oracle_lib, zkemail_rs_amd as z
        from zkemail_rs_amd import _abi as A
        import test_gpu_frontend_helper as t
        from test_gpu_verify import assert_records_equal
        engine, orc = z.Engine(0), oracle_lib.load()
        dev = torch.device("cuda", 0)
        bad, good = t.exit_emails()
        ov = t.overflow_emails()
        emails = [c[1] for c in t.geometry_emails()[::5]] + [bad[k].email for k in t.BAD_KINDS] + [c.email for c in good] + [ov["a"][0], ov["b"][0]]
        packed = A.PackedBatch(emails)
        mx = max(len(e.raw_email) for e in emails)
        dbg = A.DebugBuffers(len(emails), 2 * mx + 4096, mx + 64)
        exp = orc.verify_batch(packed, dbg, threads=4)
        cb, keep, totals = bench.device_batch(torch, packed, dev)
        runs = []
        for rep in range(2):
            out = torch.zeros(packed.n * 192, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            engine.verify_batch_device(cb, totals[0], totals[1], totals[2], out.data_ptr(), 0)
            engine.sync()
            runs.append(out.cpu().numpy().view(A.RESULT_DTYPE).copy())
        runs.append(engine.verify_batch(packed))
        assert runs[0].tobytes() == runs[1].tobytes(), "two runs of the device entry differ"
        assert_records_equal(runs[2], runs[0], None, "host entry against device entry")
        assert_records_equal(runs[0], exp, None, "device entry against the oracle")
        n_ok = 0
        for i in range(len(emails)):
            if int(exp[i]["status"]) != A.ZKE_OK:
                continue
            n_ok += 1
            H = hashlib.sha1 if int(exp[i]["flags"]) & A.F_SHA1 else hashlib.sha256
            body = bytes(dbg.canon_body[i, :int(exp[i]["canon_body_len"])])
            pre = bytes(dbg.canon_header[i, :int(exp[i]["canon_header_len"])])
            for r in runs:
                assert bytes(r[i]["body_hash"]) == H(body).digest().ljust(32, b"\\0"), i
                assert bytes(r[i]["header_hash"]) == H(pre).digest().ljust(32, b"\\0"), i
        assert n_ok > len(emails) // 2
        engine.close()
        print("side outputs ok")
    """)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ZKE_FRONT_HELPER="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "side outputs ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
