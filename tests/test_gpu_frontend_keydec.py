"""GPU parity (-m gpu) for the key stage on the helper wave of the two-wave round-0 front end (csrc/parse.hip.h, parse_kernel<true>,
ZKE_HELPER_KEYDEC): the helper decodes the RSA key and routes the signature at kernel entry, the front-end wave takes the outcome from
the mailbox behind the key barrier, and the helper stores the RSA job's modulus and exponent behind it.  Every record must be the
oracle's, field for field, for every shape of key; the by-products the key stage decides — the route (zke_debug_out.rsa_route) and,
through the RSA job the helper fills, the recovered EM block — must be those of an engine created with ZKE_FRONT_HELPER = 0, whose one
wave does the stage itself.  (EmailMeta::key_ok and even_modulus have no debug output of their own.  key_ok decides KEY_DECODE_FAIL
against every later status and whether the verdict reads EM; even_modulus decides ZKE_D_U_EVEN_MODULUS and keeps the key off the lane-group
routes: the records, the routes and the EM blocks carry both.)"""
import os

import numpy as np
import pytest

import cases
import synth
from synth import SignSpec
from zkemail_rs_amd import _abi as A
from test_gpu_frontend_helper import dirty_body
from test_gpu_rsa_edges import ROUTE_NOT_CACHED, ROUTE_NOT_TAKEN
from test_gpu_verify import assert_records_equal, em_defined, run_both

pytestmark = pytest.mark.gpu

ROUTE_QUAD, ROUTE_OCT, ROUTE_OCT9, ROUTE_NO_KERNEL = 4, 8, 16, 0x100      # RSA_F_*; keydec.hip.h rsa_route: no lane-group kernel for the size


def _engine(helper, oct9=None, **kw):
    """An engine created with ZKE_FRONT_HELPER = helper and, when given, ZKE_RSA_OCT9 = oct9 (both are read at zke_engine_create)."""
    import zkemail_rs_amd as z
    want = {"ZKE_FRONT_HELPER": helper, "ZKE_RSA_OCT9": oct9}
    old = {k: os.environ.pop(k, None) for k in want}
    for k, v in want.items():
        if v is not None:
            os.environ[k] = v
    try:
        return z.Engine(**kw)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.fixture(scope="module")
def engines():
    """(two-wave front end for every batch, one-wave front end for every batch)"""
    on, off = _engine("1"), _engine("0")
    assert all(on.front_helper(n) for n in (1, 2, 65, 130)) and not any(off.front_helper(n) for n in (1, 2, 65, 130))
    yield on, off
    on.close()
    off.close()


def _odd(bits, seed):
    n = int.from_bytes(np.random.default_rng(seed).bytes((bits + 7) // 8), "big") >> (-bits % 8)
    return n | (1 << (bits - 1)) | 1


def _long_form_e(der: bytes) -> bytes:
    """the exponent's length 3 written 81 03: a long form where the short one is due (DER forbids it), outer length adjusted"""
    assert der.endswith(b"\x02\x03\x01\x00\x01") and der[1] == 0x82
    body = der[4:-5] + b"\x02\x81\x03\x01\x00\x01"
    return b"\x30\x82" + len(body).to_bytes(2, "big") + body


def key_edges():
    """[(name, Case)]: one e-mail per shape of key.  `status` / `detail` are set where the outcome is a key failure by the
    reference's rules; everywhere else the oracle decides (status None)."""
    ks = synth.load_keys()
    k0 = cases.K()
    der = k0.pkcs1_der
    hs, body = cases._hdrs(8), cases._body(300, 12)
    out = []

    def add(name, key=None, status=None, detail=None, **kw):
        c = cases.mk(name, hs, body, key or k0, check_inter=False, **kw)
        c.status, c.detail = status, detail
        out.append((name, c))

    for nm in ("rsa1024_00", "rsa2048_03", "rsa3072_00", "rsa4096_03", "rsa2047_00", "rsa2049_00"):
        add(nm, ks[nm], A.ZKE_OK)
    add("e3", ks["rsa2047e3_00"], A.ZKE_OK)
    add("modulus_500_bits", pubkey=synth.pkcs1_pub_der(_odd(500, 1), 65537))
    add("modulus_511_bits", pubkey=synth.pkcs1_pub_der(_odd(511, 2), 65537))
    add("even_modulus", pubkey=synth.pkcs1_pub_der(k0.n - 1, 65537))
    add("even_modulus_e3", pubkey=synth.pkcs1_pub_der(k0.n - 1, 3))
    fail = dict(status=A.ZKE_KEY_DECODE_FAIL)
    add("e_9_octets", pubkey=synth.pkcs1_pub_der(k0.n, (1 << 64) + 1), detail=A.D_KEY_RANGE, **fail)
    add("e_one", pubkey=synth.pkcs1_pub_der(k0.n, 1), detail=A.D_KEY_RANGE, **fail)
    add("e_zero", pubkey=synth.pkcs1_pub_der(k0.n, 0), detail=A.D_KEY_RANGE, **fail)
    add("e_34_bits", pubkey=synth.pkcs1_pub_der(k0.n, (1 << 33) + 1), detail=A.D_KEY_RANGE, **fail)
    add("modulus_4097_bits", pubkey=synth.pkcs1_pub_der(_odd(4097, 3), 65537), detail=A.D_KEY_RANGE, **fail)
    add("der_truncated", pubkey=der[:-1], detail=A.D_KEY_DER, **fail)
    add("der_cut_in_modulus", pubkey=der[:100], detail=A.D_KEY_DER, **fail)
    add("der_trailing_byte", pubkey=der + b"\x00", detail=A.D_KEY_DER, **fail)
    add("der_outer_tag", pubkey=b"\x31" + der[1:], detail=A.D_KEY_DER, **fail)
    add("der_long_form_length", pubkey=_long_form_e(der), detail=A.D_KEY_DER, **fail)
    add("der_empty", pubkey=b"", detail=A.D_KEY_DER, **fail)
    add("key_type_dsa", key_type="dsa", detail=A.D_KEY_TYPE, **fail)
    e0 = cases.ED()[0]
    add("ed25519_32_bytes", e0, A.ZKE_OK, key_type="ed25519")
    add("ed25519_31_bytes", e0, pubkey=e0.pub[:31], key_type="ed25519", detail=A.D_KEY_DER, **fail)
    add("ed25519_key_rsa_der", pubkey=der, key_type="ed25519", detail=A.D_KEY_DER, **fail)
    return out


def good_emails(count, start=0):
    """valid e-mails under keys of both size classes, bodies the helper has something to do with"""
    ks = synth.load_keys()
    keys = [ks[n] for n in ("rsa2048_00", "rsa4096_00", "rsa1024_01", "rsa3072_00", "rsa2048_01")]
    out = []
    for j in range(start, start + count):
        bc = ("relaxed", "simple")[j % 2]
        body = dirty_body(700 + 97 * (j % 7), "crlfs") if j % 3 == 0 else cases._body(300 + 211 * (j % 5), j)
        out.append(cases.mk(f"good_{j}", cases._hdrs(40 + j), body, keys[j % len(keys)], SignSpec(body_canon=bc), check_inter=False))
    return out


def check(engines, oracle, cs, ctx, names=None):
    """records of both engines = the oracle's; route and EM of the two engines equal; the expectation written with the case holds"""
    on, off = engines
    emails = [c.email for c in cs]
    names = names or [c.name for c in cs]
    got, exp, d_on, d_orc = run_both(on, oracle, emails)
    assert_records_equal(got, exp, names, ctx)
    mx = max(len(e.raw_email) for e in emails)
    d_off = A.DebugBuffers(len(emails), 2 * mx + 4096, mx + 64)
    got_off = off.verify_batch(A.PackedBatch(emails), d_off)
    assert_records_equal(got_off, exp, names, ctx + " (one wave)")
    for i, c in enumerate(cs):
        if c.status is not None:
            assert int(got[i]["status"]) == c.status, (ctx, names[i], int(got[i]["status"]), int(got[i]["detail"]))
            if c.detail is not None:
                assert int(got[i]["detail"]) == c.detail, (ctx, names[i], int(got[i]["detail"]))
        hl, bl = int(exp[i]["canon_header_len"]), int(d_orc.full_len[i])
        assert bytes(d_on.canon_header[i, :hl]) == bytes(d_orc.canon_header[i, :hl]), (ctx, names[i])
        assert int(d_on.full_len[i]) == bl and bytes(d_on.canon_body[i, :bl]) == bytes(d_orc.canon_body[i, :bl]), (ctx, names[i])
        if em_defined(exp[i]):                  # (elsewhere the reference never reaches the RSA step)
            assert bytes(d_on.em[i]) == bytes(d_orc.em[i]), (ctx, names[i])
            assert bytes(d_on.em[i]) == bytes(d_off.em[i]), (ctx, names[i])
    return got, d_on, d_off


def same_routes(d_on, d_off, n, ctx):
    assert [int(x) for x in d_on.rsa_route[:n]] == [int(x) for x in d_off.rsa_route[:n]], \
        (ctx, [hex(int(x)) for x in d_on.rsa_route[:n]], [hex(int(x)) for x in d_off.rsa_route[:n]])


def test_key_edges_alone_beside_a_good_email_and_in_one_batch(engines, oracle):
    """Every shape of key as a batch of 1, of 2 (beside a valid e-mail, both orders in turn), all of them interleaved with valid
    e-mails in a batch of 65, and in a batch of about 130."""
    edges = key_edges()
    good = good_emails(8)
    for j, (name, c) in enumerate(edges):
        _, d_on, d_off = check(engines, oracle, [c], f"n=1 {name}")
        same_routes(d_on, d_off, 1, name)
        pair = [good[j % 8], c] if j % 2 else [c, good[j % 8]]
        _, d_on, d_off = check(engines, oracle, pair, f"n=2 {name}")
        same_routes(d_on, d_off, 2, name)
    mixed = []
    for j in range(65):
        mixed.append(edges[(j // 2) % len(edges)][1] if j % 2 else good_emails(1, 100 + j)[0])
    assert len(mixed) == 65
    got, d_on, d_off = check(engines, oracle, mixed, "n=65")
    same_routes(d_on, d_off, 65, "n=65")
    big = [c for _, c in edges] * 3 + good_emails(131 - 3 * len(edges), 200)
    big = [big[(7 * j) % len(big)] for j in range(len(big))]            # 7 is prime to the length below: a permutation
    assert len(big) == 131 and len({id(x) for x in big}) >= len(edges)
    got, d_on, d_off = check(engines, oracle, big, "n=131")
    same_routes(d_on, d_off, 131, "n=131")
    n_fail = sum(int(r["status"]) == A.ZKE_KEY_DECODE_FAIL for r in got)
    assert n_fail >= 3 * 13 and sum(int(r["status"]) == A.ZKE_OK for r in got) >= 131 - 3 * len(edges)


@pytest.mark.parametrize("oct9", ["0", "1"])
def test_routing_first_pass_wave_role_second_pass_lane_groups(oracle, oct9):
    """One batch twice on one engine: the keys are new in the first pass (route 0x200, the wave routine takes them and fills the
    cache), cached in the second — four lanes or, with ZKE_RSA_OCT9 = 1, eight lanes of nine limbs up to 2048 bits, eight lanes
    above; e = 3, an even modulus and a modulus under 512 bits are never routed.  Both front ends say the same."""
    ks = synth.load_keys()
    small, large = [ks["rsa2048_04"], ks["rsa1024_00"]], [ks["rsa4096_04"], ks["rsa3072_00"]]
    cs, want1, want2 = [], [], []
    lane = ROUTE_OCT9 if oct9 == "1" else ROUTE_QUAD
    for j in range(20):
        key = (small + large)[j % 4]
        cs.append(cases.mk(f"{key.name}_{j}", cases._hdrs(j), cases._body(200 + 13 * j, j), key, check_inter=False))
        want1.append(ROUTE_NOT_CACHED)
        want2.append(lane if key.bits <= 2048 else ROUTE_OCT)
    hs, body, k0 = cases._hdrs(8), cases._body(300, 12), cases.K()
    for name, key, pub, route in (("e3", ks["rsa2047e3_00"], None, ROUTE_NOT_TAKEN), ("even", k0, synth.pkcs1_pub_der(k0.n - 1, 65537), ROUTE_NOT_TAKEN),
                                  ("under_512", k0, synth.pkcs1_pub_der(_odd(500, 1), 65537), ROUTE_NO_KERNEL)):
        cs.append(cases.mk(name, hs, body, key, pubkey=pub, check_inter=False))
        want1.append(route)
        want2.append(route)
    for c in cs:
        c.status = None
    on, off = _engine("1", oct9, rsa_lane_groups=2), _engine("0", oct9, rsa_lane_groups=2)
    try:
        for npass, want in ((1, want1), (2, want2)):
            got, d_on, d_off = check((on, off), oracle, cs, f"oct9={oct9} pass {npass}")
            assert [int(x) for x in d_on.rsa_route[:len(cs)]] == want, (npass, [hex(int(x)) for x in d_on.rsa_route[:len(cs)]])
            same_routes(d_on, d_off, len(cs), f"pass {npass}")
            assert all(int(got[i]["status"]) == A.ZKE_OK for i in range(21)), npass
    finally:
        on.close()
        off.close()


def precedence_cases():
    """a key that does not decode, combined with failures in front of the key site (they win) and behind it (the key wins)"""
    k0 = cases.K()
    hs, body = cases._hdrs(8), cases._body(300, 12)
    bad_key = dict(pubkey=b"\x30\x03\x02\x01", check_inter=False)
    key_wins = dict(status=A.ZKE_KEY_DECODE_FAIL, detail=A.D_KEY_DER, **bad_key)
    mp = b'multipart/alternative; boundary="=_b0"'
    mime_bad = b"preamble\r\n--=_b0\r\n Content-Type: text/plain; charset=utf-8\r\n\r\nplain text\r\n--=_b0--\r\n"
    mk = cases.mk
    return [
        mk("key+unparsable_header", hs, body, k0, mutate=lambda r: b" bad start\r\n" + r, status=A.ZKE_PARSE_FAIL, detail=A.D_HDR_LEADING_SPACE, **bad_key),
        mk("key+too_many_headers", [(b"X-Filler-%d" % i, b"v") for i in range(260)] + cases._hdrs(30), cases._body(200, 30), k0,
           status=A.ZKE_UNSUPPORTED, detail=A.D_U_TOO_MANY_HEADERS, **bad_key),
        mk("key+mime_structure", cases._with_ctype(cases._hdrs(11), mp), mime_bad, k0, status=A.ZKE_PARSE_FAIL, detail=A.D_SUBPART_LEADING_SPACE, **bad_key),
        mk("key+kelvin_domain", cases._hdrs(7), cases._body(100, 11), k0, SignSpec(domain="example.kom"), from_domain="example.\u212Aom", **key_wins),
        mk("key+no_signature", hs, body, k0, mutate=lambda r: r[r.find(b"Received:"):], **key_wins),
        mk("key+bad_b", hs, body, k0, SignSpec(fold_sig=False), mutate=lambda r: r.replace(b" b=", b" b=!", 1), **key_wins),
        mk("key+body_hash", hs, body, k0, corrupt="body", **key_wins),
        mk("key_type+kelvin_domain", cases._hdrs(7), cases._body(100, 11), k0, SignSpec(domain="example.kom"), from_domain="example.\u212Aom", key_type="dsa",
           status=A.ZKE_KEY_DECODE_FAIL, detail=A.D_KEY_TYPE, check_inter=False),
        # and the later failures alone, under a good key: what the key failure wins over
        mk("kelvin_domain", cases._hdrs(7), cases._body(100, 11), k0, SignSpec(domain="example.kom"), from_domain="example.\u212Aom",
           status=A.ZKE_UNSUPPORTED, detail=A.D_U_DOMAIN_FOLD, check_inter=False),
        mk("body_hash", hs, body, k0, corrupt="body", status=A.ZKE_DKIM_NOT_PASS, detail=A.D_BODY_HASH_MISMATCH, check_inter=False),
    ]


def test_precedence_with_the_helper_live_on_every_exit(engines, oracle):
    """parse, MIME, key type, key decode, domain, signature — in that order, one e-mail per combination beside valid e-mails"""
    pc = precedence_cases()
    good = good_emails(len(pc) + 1, 300)
    batch = [x for pair in zip(good, pc) for x in pair] + [good[-1]]
    check(engines, oracle, batch, "precedence")
    for c in pc:
        check(engines, oracle, [c], "precedence n=1 " + c.name)


def test_slot_reuse_leaves_nothing_of_the_previous_rsa_job(engines, oracle):
    """valid batch, a batch of the same size failing before, at and after the key site, the valid batch again: each equals the
    oracle, records and EM — the helper stores a job's key fields exactly when the front-end wave came through the key site"""
    good = good_emails(65, 400)
    pc = precedence_cases()
    edges = [c for _, c in key_edges()]
    failing = [(pc + edges)[j % (len(pc) + len(edges))] for j in range(65)]
    for rep, batch in enumerate((good, failing, good)):
        got, _, _ = check(engines, oracle, batch, f"slot reuse {rep}")
        if rep != 1:
            assert all(int(r["status"]) == A.ZKE_OK for r in got)


def test_both_entry_points_three_times_over():
    """the mixed batch (key edges, precedence, valid) three times through the device entry and three times through zke_verify_batch:
    identical records, equal to the oracle's.  In a subprocess so that torch, which owns the device buffers, initialises HIP first."""
    import subprocess, sys, textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent(f"""
        import sys
        sys.path.insert(0, {root!r}); sys.path.insert(0, {os.path.join(root, 'tests')!r})
        import numpy as np, torch
        torch.zeros(1, device="cuda")
        import bench, oracle_lib, zkemail_rs_amd as z
        from zkemail_rs_amd import _abi as A
        import test_gpu_frontend_keydec as t
        from test_gpu_verify import assert_records_equal
        engine, orc = z.Engine(0), oracle_lib.load()
        assert engine.front_helper(130)
        dev = torch.device("cuda", 0)
        cs = [c for _, c in t.key_edges()] + t.precedence_cases() + t.good_emails(90, 500)
        cs = [cs[(11 * j) % len(cs)] for j in range(len(cs))]
        emails = [c.email for c in cs]
        packed = A.PackedBatch(emails)
        exp = orc.verify_batch(packed, None, threads=4)
        cb, keep, totals = bench.device_batch(torch, packed, dev)
        runs = []
        for rep in range(3):
            out = torch.zeros(packed.n * 192, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            engine.verify_batch_device(cb, totals[0], totals[1], totals[2], out.data_ptr(), 0)
            engine.sync()
            runs.append(out.cpu().numpy().view(A.RESULT_DTYPE).copy())
        for rep in range(3):
            runs.append(engine.verify_batch(packed))
        for k, r in enumerate(runs):
            assert_records_equal(r, exp, [c.name for c in cs], f"run {{k}} against the oracle")
        assert all(runs[0].tobytes() == r.tobytes() for r in runs[1:3]), "runs of the device entry differ"
        assert sum(int(r["status"]) == A.ZKE_OK for r in runs[0]) >= 90
        engine.close()
        print("entry points ok", len(emails))
    """)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ZKE_FRONT_HELPER="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "entry points ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
