"""GPU (-m gpu): the lane-group RSA routine (rsa_quad.hip.h rsa_group_wave<4> / <8>) after its per-step bookkeeping and its
EMSA walk were trimmed: the masks of the quotient digit and of the finished column moved behind their DPP moves, the FF run and
the zeros above k checked on limbs and only the boundary bytes walked.

Reached as tests/test_gpu_rsa_limb29.py reaches it: an engine with lane groups forced, every batch twice so that the second
pass takes the lane groups (route asserted), EM read from the debug buffers.  The debug passes write every EM byte out, which
keeps the full byte walk (beside the limb compares); a third pass WITHOUT debug buffers runs what production runs — limbs and
boundary bytes alone — and its records must equal the oracle's too.  tests/test_rsa_group_trim_model.py is the CPU model."""
import base64
import random

import numpy as np
import pytest

import synth
from synth import SignSpec
from test_gpu_rsa_edges import edge_emails, edge_key, fresh_engine, make_email, run_twice      # noqa: F401  (the shared route)
from test_gpu_rsa_limb29 import Engines
from test_gpu_verify import assert_records_equal, run_both
from zkemail_rs_amd import _abi as A

pytestmark = pytest.mark.gpu

QL, QBITS = 18, 29
LANE_BITS = QL * QBITS                                   # 522
TLEN = 51                                                # DigestInfo + SHA-256 digest


@pytest.fixture(scope="module")
def engines():
    e = Engines()
    yield e
    e.close()


def production_pass(eng, oracle, items, ctx):
    """no debug buffers: the shape verdict comes from the limb classes and the boundary walk alone"""
    got, exp, _, _ = run_both(eng, oracle, [it[0] for it in items], dbg=False)
    assert_records_equal(got, exp, None, ctx + " production pass")
    return got


@pytest.mark.parametrize("name,full", [("rsa2048_03", 16), ("rsa4096_03", 8)])
def test_one_full_wave(engines, oracle, name, full):
    """16 four-lane (8 eight-lane) signatures s = t^d mod n of random t: every digit lane of every block carries its own data in
    every quad of the wave.  EM = t; then one e-mail more, so that a second, nearly empty wave runs."""
    key = synth.load_keys()[name]
    eng = engines.of(key)
    rng, prng = np.random.default_rng(full), random.Random(full)
    pool = []
    for i in range(full + 1):
        t = prng.randrange(key.n)
        item = make_email(rng, i, key, pow(t, key.d, key.n).to_bytes(key.k, "big")) + (f"random{i}",)
        assert item[1] == t.to_bytes(key.k, "big")
        pool.append(item)
    run_twice(eng, oracle, pool[:2], [key] * 2, f"{name} warm-up")
    for size in (full, full + 1):
        run_twice(eng, oracle, pool[:size], [key] * size, f"{name} x {size}")
        got = production_pass(eng, oracle, pool[:size], f"{name} x {size}")
        assert all(int(r["status"]) == A.ZKE_DKIM_NOT_PASS for r in got)          # a random EM has no EMSA shape


def corrupt_positions(k):
    """little-endian byte positions of EM: {tag: position}"""
    pos = {"digestinfo-low": 32, "digestinfo-high": 50, "separator": 51, "first-ff": 52, "last-ff": k - 3, "01": k - 2, "top-00": k - 1}
    for p in range(1, 8):
        b = LANE_BITS * p // 8                           # the byte that holds bit 522 p, and its neighbours
        for q in (b - 1, b, b + 1):
            if TLEN + 1 <= q < k - 2:
                pos[f"lane{p}-boundary-byte{q}"] = q
    t = (8 * (TLEN + 1) + QBITS - 1) // QBITS + 4        # an interior limb of lane 1 well inside the run, its middle byte
    assert QL < t < 2 * QL - 1 and (QBITS * t + 14) // 8 < k - 3
    pos["interior-limb"] = (QBITS * t + 14) // 8
    return pos


def with_signature(raw, sig):
    a = raw.find(b" b=") + 3
    z = raw.find(b"\r\nReceived", a)
    return raw[:a] + base64.b64encode(sig) + raw[z:]


@pytest.mark.parametrize("name", ["rsa1024_00", "rsa2047_00", "rsa2048_03", "rsa3072_00", "rsa4096_03"])
def test_padding_corrupted_at_one_position(engines, oracle, name):
    """One signed e-mail, re-emitted with b= = EM'^d mod n for EM' = its EM with one byte changed in front of the digest (the
    header hash does not cover b=, and the digest in EM' is right): verified as signed, the oracle's failing record for every
    corrupted copy — whether a limb compare or the byte walk is what sees the byte."""
    key = synth.load_keys()[name]
    eng = engines.of(key)
    rng = np.random.default_rng(key.bits)
    raw, it = synth.sign_email(synth.std_headers(rng, 0, "example.com"), synth.ascii_body(rng, 333), key, SignSpec(domain="example.com"))
    em = int.from_bytes(it["em"], "big")
    k = key.k
    items = [(A.Email("example.com", raw, A.PublicKey(key.pkcs1_der)), it["em"], "valid")]
    cases = [(tag, em ^ (0x01 << (8 * q))) for tag, q in corrupt_positions(k).items()]
    # (no case with a byte at or above k set: such a value is at least 2^(8k) > n for a k-byte modulus, so no signature gives it;
    # the limbs above bit 8k are covered by the CPU model's bit flips)
    for tag, x in cases:
        assert x < key.n, tag
        sig = pow(x, key.d, key.n).to_bytes(k, "big")
        items.append((A.Email("example.com", with_signature(raw, sig), A.PublicKey(key.pkcs1_der)), x.to_bytes(k, "big"), tag))
    assert len(items) >= 12
    keys = [key] * len(items)
    run_twice(eng, oracle, items[:1], keys[:1], f"{name} warm-up")
    for ctx, got in (("debug", run_both(eng, oracle, [i[0] for i in items])[0]), ("production", production_pass(eng, oracle, items, name))):
        assert int(got[0]["status"]) == A.ZKE_OK, (name, ctx)
        for i in range(1, len(items)):
            assert int(got[i]["status"]) == A.ZKE_DKIM_NOT_PASS, (name, ctx, items[i][2])
    run_twice(eng, oracle, items, keys, name)             # EM of every copy from the debug buffers, records against the oracle
