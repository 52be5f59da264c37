"""-m gpu: the verdict launch (verdict.hip.h, canon.hip.h) decides an e-mail from what its lane loaded in one go — the whole
EmailMeta as 16-byte words, the record's two hashes, the external-input flag.  Every way through the status cascade sits side by
side in one wave of 16 e-mails here, so that each lane of the wave takes another one:

  a passing rsa-sha256 e-mail; rsa-sha1 (28 base64 characters of bh=, the pad in the seventh group, five digest limbs); Ed25519;
  a flipped body byte (bh mismatch) and a flipped header byte (EM well-formed, digest limbs differ) for each of the three;
  bh= one character short and one long (bh_len), and with its last character changed (the pad group alone differs);
  a b= that is no base64; a passing e-mail with a null external input, and a failing one (the flag must not show);
  an e-mail whose first same-domain signature fails and whose second passes (ST_PENDING, next_round, the lane reads again), and
  one with three failing ones in front.

Batches of 1 (each kind alone), 17 (one lane in the second wave) and 65 (five waves, one lane in the last), every field of every
record against the oracle's; and the same batches on an engine with max_sig_rounds = 1, where the e-mails that need a second
round are reported as unsupported and every other record is still the oracle's.

The b= side of the strict base64 decoder (decode_sig over b64_quad, csrc/keydec.hip.h) has kinds of its own, named b_*: every
way a quad can be malformed, in the first, second and third step of the decoder's loop over 64 quads (an RSA-2048 b= has 86
quads, an RSA-3072 one 128 and no padding, an RSA-4096 one 171).  Each alone, and all kinds side by side in one batch."""
import base64
import binascii

import numpy as np
import pytest

import cases
from cases import K, SignSpec, _body, _hdrs, mk
from test_gpu_verify import assert_records_equal
from zkemail_rs_amd import _abi as A

pytestmark = pytest.mark.gpu


def _bh_edit(edit):
    def f(raw):
        i = raw.find(b" bh=") + 4
        j = raw.find(b";", i)
        return raw[:i] + edit(raw[i:j]) + raw[j:]
    return f


B64 = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"


def _b_value(raw):
    """the b= value of the first DKIM-Signature header (written unfolded: SignSpec(fold_sig=False))"""
    h = raw.find(b"DKIM-Signature:")
    i = raw.find(b"\r\n b=", h) + 5           # the signer puts b= last, on a continuation line of its own
    j = raw.find(b"\r\n", i)
    assert h >= 0 and i > h + 5 and raw[j + 2:j + 3] not in (b" ", b"\t") and b"\r\n\r\n" not in raw[h:j]
    return i, j


def _b_edit(edit):
    def f(raw):
        i, j = _b_value(raw)
        return raw[:i] + edit(raw[i:j]) + raw[j:]
    return f


def _put(pos, new):
    """the character at `pos` of the value replaced: by `new`, or (new = None) by the one whose six bits have bit 0 set as well"""
    def f(v):
        p = pos % len(v)
        c = new if new is not None else B64[B64.index(v[p]) | 1:][:1]
        assert c != v[p:p + 1]
        return v[:p] + c + v[p + 1:]
    return f


def _b_kinds():
    """[(name, key, edit of the unfolded b= value)]: one small e-mail each.  `*` is a valchar of the tag list outside the alphabet."""
    q = lambda quad, pos: 4 * quad + pos
    out = [("b_length_not_a_multiple_of_4", "rsa2048_00", lambda v: v[:-2]),                  # 86 quads, two pads: both dropped
           ("b_one_pad_trailing_bits", "rsa1024_00", _put(-2, None)),                         # 128 bytes: 43 quads, one pad
           ("b_two_pads_trailing_bits", "rsa2048_00", _put(-3, None)),
           ("b_pad_inside_a_middle_quad", "rsa2048_00", _put(q(40, 2), b"="))]
    out += [(f"b_bad_character_position_{p}", "rsa2048_00", _put(q(10, p), b"*")) for p in range(4)]
    out += [("b_bad_character_quad_63", "rsa2048_00", _put(q(63, 1), b"*")),                  # the last lane of the loop's first step
            ("b_bad_character_quad_64", "rsa2048_00", _put(q(64, 2), b"*")),                  # the first lane of its second step
            ("b_3072_no_padding", "rsa3072_00", None),                                        # 384 bytes: 128 quads, valid
            ("b_3072_bad_character_quad_127", "rsa3072_00", _put(q(127, 3), b"*")),           # its last quad: the second step's last lane
            ("b_4096_bad_character_quad_128", "rsa4096_00", _put(q(128, 0), b"*"))]           # 171 quads: the third step's first lane
    return out


def _is_sig_b64(v):
    """D_SIG_B64, derived here: base64.b64decode(validate=True) rejects the value, or the bits behind its last byte are not zero"""
    try:
        base64.b64decode(v, validate=True)
    except binascii.Error:
        return True
    pad = len(v) - len(v.rstrip(b"="))
    return pad > 0 and (B64.index(v[-pad - 1]) & (15 if pad == 2 else 3)) != 0


def _kinds():
    """[(name, Email, needs a second signature round)]"""
    by_name = {c.name: c for c in cases.build_cases()}
    k0 = K()
    picked = ["pass_relaxed_relaxed", "pass_rsa_sha1_relaxed", "pass_ed25519_relaxed_relaxed",
              "fail_body_flipped", "fail_header_flipped", "fail_rsa_sha1_body", "fail_rsa_sha1_header",
              "fail_ed25519_body", "fail_ed25519_header", "fail_sig_b64_unpadded", "ext_null"]
    out = [(nm, by_name[nm].email, False) for nm in picked]
    out.insert(3, ("second_signature_passes", cases.multi_signature_case(1).email, True))
    fail = dict(status=A.ZKE_DKIM_NOT_PASS, detail=A.D_BODY_HASH_MISMATCH, check_inter=False)
    for nm, edit in (("bh_one_short", lambda v: v[:-1]), ("bh_one_long", lambda v: v + b"A"),
                     ("bh_last_character", lambda v: v[:-1] + b"A"), ("bh_first_character", lambda v: (b"B" if v[:1] != b"B" else b"C") + v[1:])):
        out.append((nm, mk(nm, _hdrs(8), _body(300, 12), k0, mutate=_bh_edit(edit), **fail).email, False))
    out.append(("bh_one_short_sha1", mk("bh_one_short_sha1", _hdrs(8), _body(300, 12), k0, SignSpec(algo="rsa-sha1"), mutate=_bh_edit(lambda v: v[:-1]), **fail).email, False))
    c = mk("ext_null_on_a_failing_email", _hdrs(9), _body(100, 2), k0, corrupt="header", status=A.ZKE_DKIM_NOT_PASS, detail=A.D_SIG_MISMATCH, check_inter=False)
    c.email.external_inputs = [A.ExternalInput("name", None, 8)]
    out.append((c.name, c.email, False))
    out.append(("fourth_signature_passes", cases.multi_signature_case(3).email, True))
    for nm, key, edit in _b_kinds():
        kw = dict(status=A.ZKE_DKIM_NOT_PASS, detail=A.D_SIG_B64, check_inter=False, mutate=_b_edit(edit)) if edit else {}
        out.append((nm, mk(nm, _hdrs(8), _body(300, 12), K(key), SignSpec(fold_sig=False), **kw).email, False))
    assert [nm for nm, _, _ in out[:16]].count("second_signature_passes") == 1      # the first sixteen are the first wave of the batch of 17
    return out


@pytest.fixture(scope="module")
def kinds():
    return _kinds()


@pytest.fixture(scope="module")
def batches(oracle, kinds):
    """[(names, PackedBatch, the oracle's records, which e-mails need a second round)] — made once, read by both tests"""
    out = []

    def add(picks):
        names, emails, later = zip(*picks)
        p = A.PackedBatch(list(emails))
        out.append((names, p, oracle.verify_batch(p, threads=4), np.array(later)))
    for k in kinds:
        add([k])                                                                          # n = 1
    add([kinds[j % len(kinds)] for j in range(17)])                                       # a full wave of different kinds + one lane
    add([kinds[(j + 16 * (j // 16) + 3) % len(kinds)] for j in range(65)])                # five waves, each lane another kind per wave
    add(kinds)                                                                            # every kind once, the b_* ones side by side
    return out


def test_the_kinds_are_what_they_are_meant_to_be(batches, kinds):
    """the oracle's verdicts: the cascade's branches are all there"""
    seen = {}
    for names, _, exp, _ in batches[:len(kinds)]:
        seen[names[0]] = (int(exp[0]["status"]), int(exp[0]["detail"]))
    ok, fail = (A.ZKE_OK, 0), A.ZKE_DKIM_NOT_PASS
    for nm in ("pass_relaxed_relaxed", "pass_rsa_sha1_relaxed", "pass_ed25519_relaxed_relaxed", "second_signature_passes", "fourth_signature_passes"):
        assert seen[nm] == ok, nm
    for nm in ("fail_body_flipped", "fail_rsa_sha1_body", "fail_ed25519_body", "bh_one_short", "bh_one_long", "bh_last_character",
               "bh_first_character", "bh_one_short_sha1"):
        assert seen[nm] == (fail, A.D_BODY_HASH_MISMATCH), nm
    for nm in ("fail_header_flipped", "fail_rsa_sha1_header", "fail_ed25519_header", "ext_null_on_a_failing_email"):
        assert seen[nm] == (fail, A.D_SIG_MISMATCH), nm
    assert seen["fail_sig_b64_unpadded"] == (fail, A.D_SIG_B64)
    assert seen["ext_null"][0] == A.ZKE_EXTERNAL_INPUT_NULL
    # the b= kinds: D_SIG_B64 where Python's strict decoder (and the trailing-bits rule) says so, the valid one passes
    n_b64 = 0
    for nm, em, _ in kinds:
        if nm.startswith("b_"):
            i, j = _b_value(em.raw_email)
            b64 = _is_sig_b64(em.raw_email[i:j])
            assert (seen[nm] == (fail, A.D_SIG_B64)) == b64, nm
            assert b64 == (nm != "b_3072_no_padding"), nm
            n_b64 += b64
    assert n_b64 == 12 and seen["b_3072_no_padding"] == ok


def test_every_record_equals_the_oracles(engine, batches):
    for names, p, exp, _ in batches:
        for rep in range(2):              # the second time the RSA keys are cached: the lane groups leave em_ok / em_tail, not the wave routine
            got = engine.verify_batch(p)
            assert_records_equal(got, exp, names, f"n = {p.n}, pass {rep}")


def test_one_signature_round_only(batches):
    """max_sig_rounds = 1: an e-mail whose first candidate fails while another is untried is unsupported (never guessed), in the
    same launch and the same waves as the others, whose records stay the oracle's"""
    import zkemail_rs_amd as z
    eng = z.Engine(max_sig_rounds=1)
    try:
        for names, p, exp, later in batches:
            for rep in range(2):
                got = eng.verify_batch(p)
                keep = np.flatnonzero(~later)
                assert_records_equal(got[keep], exp[keep], [names[i] for i in keep], f"one round, n = {p.n}, pass {rep}")
                for i in np.flatnonzero(later):
                    assert (int(got[i]["status"]), int(got[i]["detail"])) == (A.ZKE_UNSUPPORTED, A.D_U_TOO_MANY_SIGS), names[i]
                    assert not np.asarray(got[i]["from_domain_hash"]).any() and not np.asarray(got[i]["public_key_hash"]).any(), names[i]
    finally:
        eng.close()
