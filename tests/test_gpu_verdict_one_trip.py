"""GPU parity (-m gpu) for the verdict launch's one-trip path (csrc/verdict.hip.h, ed_verdict_kernel, ZKE_VERDICT_ONE_TRIP): a wave
requests every load of its 16 verdicts at kernel entry, decides them in place when no e-mail of it has Ed25519 work, and leaves
for one call — the Ed25519 stage, every load again, the later signature rounds — when one has, or when a verdict left an e-mail
pending.  Every record must be the CPU oracle's, field for field, whichever way the wave went.

Batches of 1, 16, 17 and 33 e-mails: a wave with a single active lane, a full one, and both beside each other.  The e-mails of one
wave are mixed, one of each outcome the verdict lane can reach (`kinds`).  The count of e-mails left pending has no output in the
ABI: the records of the two-signature e-mails, which are written by the later round, carry it."""
import numpy as np
import pytest

import cases
import synth
from synth import SignSpec
from zkemail_rs_amd import _abi as A
from test_gpu_verify import assert_records_equal, run_both

pytestmark = pytest.mark.gpu

ED_KINDS = ("ed_valid", "ed_key_not_a_point", "ed_sig_63_bytes")


def _both_signatures_fail() -> cases.Case:
    """two same-domain signatures: the first over another body, the second over this body before a byte of it changed"""
    c = cases.multi_signature_case(1)
    raw = c.email.raw_email
    at = raw.index(b"\r\n\r\n") + 4
    k = next(j for j in range(at, len(raw)) if raw[j:j + 1].isalnum())
    flipped = raw[:k] + (b"#" if raw[k:k + 1] != b"#" else b"%") + raw[k + 1:]
    return cases.Case("both_signatures_fail", A.Email("example.com", flipped, c.email.public_key), A.ZKE_DKIM_NOT_PASS,
                      A.D_BODY_HASH_MISMATCH, None, check_inter=False)


@pytest.fixture(scope="module")
def kinds():
    """{name: Case}, one e-mail per outcome; `status` / `detail` by the reference's rules, independent of the oracle"""
    k0, e0 = cases.K(), cases.ED()[0]
    hs, body = cases._hdrs(8), cases._body(300, 12)
    mk, NP = cases.mk, A.ZKE_DKIM_NOT_PASS
    ed = dict(key_type="ed25519", check_inter=False)
    out = {
        "rsa_valid": mk("rsa_valid", hs, body, k0),
        "body_flipped": mk("body_flipped", hs, body, k0, corrupt="body", status=NP, detail=A.D_BODY_HASH_MISMATCH, check_inter=False),
        "header_flipped": mk("header_flipped", hs, body, k0, corrupt="header", status=NP, detail=A.D_SIG_MISMATCH, check_inter=False),
        "bad_b64_b": mk("bad_b64_b", hs, body, k0, SignSpec(fold_sig=False), mutate=lambda r: r.replace(b"==\r\nReceived", b"=\r\nReceived", 1),
                        status=NP, detail=A.D_SIG_B64, check_inter=False),
        "even_modulus": mk("even_modulus", hs, body, k0, pubkey=synth.pkcs1_pub_der(k0.n - 1, 65537), status=A.ZKE_UNSUPPORTED,
                           detail=A.D_U_EVEN_MODULUS, check_inter=False),
        "sha1": mk("sha1", hs, body, k0, SignSpec(algo="rsa-sha1")),
        "ext_null": mk("ext_null", cases._hdrs(9), cases._body(100, 2), k0, status=A.ZKE_EXTERNAL_INPUT_NULL, check_inter=False),
        "ed_valid": mk("ed_valid", hs, body, e0, **ed),
        "ed_key_not_a_point": mk("ed_key_not_a_point", hs, body, e0, pubkey=cases._not_a_point(), status=A.ZKE_KEY_DECODE_FAIL,
                                 detail=A.D_KEY_ED25519_POINT, **ed),
        "ed_sig_63_bytes": mk("ed_sig_63_bytes", hs, body, e0, SignSpec(fold_sig=False), mutate=lambda r: cases._replace_sig(r, b"\x07" * 63),
                              status=NP, detail=A.D_SIG_MISMATCH, **ed),
        "second_signature_passes": cases.multi_signature_case(1),
        "both_signatures_fail": _both_signatures_fail(),
    }
    out["ext_null"].email.external_inputs = [A.ExternalInput("name", None, 8)]
    for name, c in out.items():
        c.name = name
    return out


def check(engine, oracle, cs, ctx):
    got, exp, _, _ = run_both(engine, oracle, [c.email for c in cs], dbg=False)
    names = [c.name for c in cs]
    assert_records_equal(got, exp, names, ctx)
    for i, c in enumerate(cs):                      # and both equal the expectation written with the case
        assert int(got[i]["status"]) == c.status, (ctx, i, c.name, int(got[i]["status"]), int(got[i]["detail"]))
        if c.detail is not None:
            assert int(got[i]["detail"]) == c.detail, (ctx, i, c.name, int(got[i]["detail"]))
    return got


def test_every_kind_alone(engine, oracle, kinds):
    """n = 1: one active lane, every outcome in turn — the in-place verdict, the Ed25519 call, the call for a later round"""
    for name, c in kinds.items():
        check(engine, oracle, [c], f"n=1 {name}")


@pytest.mark.parametrize("n", [16, 17, 33])
def test_mixed_waves(engine, oracle, kinds, n):
    """every kind in one wave; for n = 17 and 33 the wave of a single e-mail holds, in turn, an RSA e-mail, an Ed25519 e-mail and
    a two-signature e-mail, beside full waves of all kinds"""
    order = list(kinds)
    assert len(order) == 12
    for last in ("rsa_valid", "ed_valid", "second_signature_passes") if n % 16 == 1 else ("rsa_valid",):
        cs = [kinds[order[(5 * j) % 12]] for j in range(n - 1)] + [kinds[last]]      # 5 is prime to 12: each run of 12 holds every kind
        assert len(cs) == n and {c.name for c in cs[:16]} == set(order) | {cs[15].name}
        check(engine, oracle, cs, f"n={n} last={last}")


def test_rsa_only_waves_take_no_ed25519_kind(engine, oracle, kinds):
    """two waves without an Ed25519 e-mail: RSA outcomes only, the two-signature e-mails among them (the call for the later round
    from the in-place verdict) — and the same batch without those (no call at all)"""
    rsa = [n for n in kinds if n not in ED_KINDS]
    for ctx, names in (("with later rounds", rsa), ("no call", [n for n in rsa if "signature" not in n])):
        cs = [kinds[names[(4 * j + j // len(names)) % len(names)]] for j in range(32)]
        assert {c.name for c in cs} == set(names)
        check(engine, oracle, cs, f"rsa only, {ctx}")


def test_in_place_and_called_verdicts_write_the_same_bytes(engine, oracle, kinds):
    """A wave of RSA e-mails only beside a wave that holds the same e-mails and the batch's only Ed25519 e-mail: the first decides in
    place, the second through the call.  The records of the same e-mail are the same bytes in both, and the oracle's."""
    rsa = [n for n in kinds if n not in ED_KINDS and "signature" not in n]
    wave = [kinds[rsa[j % len(rsa)]] for j in range(15)]
    cs = wave + [kinds["rsa_valid"]] + wave + [kinds["ed_valid"]]
    assert len(cs) == 32 and not any(c.name in ED_KINDS for c in cs[:16]) and sum(c.name in ED_KINDS for c in cs[16:]) == 1
    got = check(engine, oracle, cs, "lean wave beside full wave")
    for j in range(15):
        assert np.asarray(got[j:j + 1]).tobytes() == np.asarray(got[16 + j:17 + j]).tobytes(), (j, cs[j].name)
    assert int(got[31]["status"]) == A.ZKE_OK
