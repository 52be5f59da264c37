"""GPU (-m gpu): both RSA modexp routines on the operands of tests/rsa_edge_cases.py, against Python's pow and the oracle.

  * The one-signature-per-wave routine (rsa.hip.h mont_core_64 / 128 under rsa_kernel.hip.h rsa_wave_any), through the
    building-block entry zke_rsa_modexp_batch: one launch per container size and every case in one 512-byte launch.
  * The lane-group routine (rsa_quad.hip.h rsa_group_wave<4> / <8>), which has no building-block entry, through the
    pipeline with rsa_lane_groups = 2: each batch runs twice — the first time the wave routine takes the signatures and
    fills the key cache, the second time the front end routes them to four lanes (512..2048 bits) or eight (..4096).
The CPU models of tests/test_rsa_wave_model.py show that these operands reach the routines' data-dependent paths."""
import base64
import random

import numpy as np
import pytest

import rsa_edge_cases as rc
import synth
from synth import SignSpec
from test_gpu_verify import assert_records_equal, run_both
from zkemail_rs_amd import _abi as A

pytestmark = pytest.mark.gpu

KEY_NAMES = ("rsa1024_00", "rsa1025_00", "rsa2047_00", "rsa2047e3_00", "rsa2048_03", "rsa2049_00", "rsa3071_00",
             "rsa4095_00", "rsa4096_03")
ROUTE_NOT_CACHED, ROUTE_SLOT_TAKEN, ROUTE_NOT_TAKEN = 0x200, 0x400, 0x800       # keydec.hip.h rsa_route / the e != 65537 case


def key_cache_slot(n):
    """rsa.hip.h key_cache_slot of the modulus' two low 32-bit limbs"""
    n0, n1 = n & 0xFFFFFFFF, (n >> 32) & 0xFFFFFFFF
    return ((n0 * 0x9E3779B1 + n1 * 0x85EBCA77) & 0xFFFFFFFF) >> 20


def block_cases():
    return rc.wave_cases() + rc.key_cases(synth.load_keys(), KEY_NAMES)


def check_block_launch(engine, oracle, cases, nbytes):
    cases = [c for c in cases if c[2] < 1 << (8 * nbytes) and c[0] < 1 << (8 * nbytes)]
    assert cases
    sigs = [s.to_bytes(nbytes, "big") for _, _, s, _ in cases]
    mods = [n.to_bytes(nbytes, "big") for n, _, _, _ in cases]
    em, ok = engine.rsa_modexp_batch(sigs, mods, [e for _, e, _, _ in cases], nbytes)
    accepted = 0
    for (n, e, s, tag), sig, mod, g, o in zip(cases, sigs, mods, em, ok):
        want_ok = n & 1 == 1 and n.bit_length() >= 2 and s < n          # the entry's ok: s < n, n odd, n of 2 bits or more
        assert int(o) == int(want_ok), (nbytes, tag)
        rcode, exp = oracle.rsa_modexp(sig, mod, e)
        if not want_ok:
            assert rcode != 0, (nbytes, tag)
            continue
        want = pow(s, e, n).to_bytes(nbytes, "big")
        assert rcode == 0 and exp == want, ("oracle", nbytes, tag)
        assert bytes(g) == want, (nbytes, tag)
        accepted += 1
    return accepted


@pytest.mark.parametrize("container", [256, 512])
def test_wave_routine_edge_cases_per_container(engine, oracle, container):
    """every case whose modulus fits the container and needs it (<= 2048 bits: 256 bytes; 2049..4096: 512), one launch"""
    cases = [c for c in block_cases() if rc.container_bits(c[0].bit_length()) == 8 * container]
    assert check_block_launch(engine, oracle, cases, container) >= 200


def test_wave_routine_edge_cases_mixed_launch(engine, oracle):
    """all cases, every size and exponent, in one 512-byte launch"""
    cases = block_cases()
    assert {e for _, e, _, _ in cases} == set(rc.WAVE_EXPONENTS)
    assert check_block_launch(engine, oracle, cases, 512) >= 800


# ---- the lane-group routine through the pipeline ---------------------------------------------------------------------

class EdgeKey(synth.RsaKey):
    """a modulus without its factors: the e-mail is signed with a placeholder and its b= replaced by an edge value"""

    def sign_em(self, em):
        return b"\x01" * self.k


def edge_key(tag, n, e=65537):
    return EdgeKey(tag, n.bit_length(), n, e, 0, 0, 0, synth.pkcs1_pub_der(n, e))


def make_email(rng, i, key, sig=None):
    """(email, expected EM or None when rsa 0.9.6 rejects the signature before the arithmetic, valid: b= left as signed)"""
    body = synth.ascii_body(rng, 300 + 7 * (i % 50))
    raw, it = synth.sign_email(synth.std_headers(rng, i, "example.com"), body, key, SignSpec(domain="example.com"))
    if sig is None:
        want = it["em"]
    else:
        a = raw.find(b" b=") + 3
        z = raw.find(b"\r\nReceived", a)
        raw = raw[:a] + base64.b64encode(sig) + raw[z:]
        s = int.from_bytes(sig, "big")
        want = pow(s, key.e, key.n).to_bytes(key.k, "big") if len(sig) == key.k and s < key.n else None
    return A.Email("example.com", raw, A.PublicKey(key.pkcs1_der)), want


def edge_emails(rng, key, start, sigs=None):
    """one e-mail per edge signature of the key (accepted and rejected values, b= a byte short, b= a byte long with a
    leading zero), and a valid signature when the key is real"""
    out = []
    for s, tag in sigs if sigs is not None else rc.signatures(key.n, rng):
        if s < 1 << (8 * key.k):
            out.append(make_email(rng, start + len(out), key, s.to_bytes(key.k, "big")) + (tag,))
    s = (int.from_bytes(rng.bytes(key.k), "big") % key.n).to_bytes(key.k, "big")
    out.append(make_email(rng, start + len(out), key, s[1:]) + ("short",))
    out.append(make_email(rng, start + len(out), key, b"\0" + s) + ("long",))
    if not isinstance(key, EdgeKey):
        out.append(make_email(rng, start + len(out), key) + ("valid",))
    return out


def check_pass(got, exp, d_gpu, d_orc, items, keys, ctx):
    assert_records_equal(got, exp, None, ctx)
    for i, ((_, want, tag), key) in enumerate(zip(items, keys)):
        if want is None:
            assert int(got[i]["status"]) == A.ZKE_DKIM_NOT_PASS and int(got[i]["detail"]) == A.D_SIG_MISMATCH, (ctx, key.name, tag)
            assert not d_gpu.em[i].any(), (ctx, key.name, tag)
        else:
            assert bytes(d_gpu.em[i, :key.k]) == want, (ctx, key.name, tag)
            assert not d_gpu.em[i, key.k:].any(), (ctx, key.name, tag)
            if tag == "valid":
                assert int(got[i]["status"]) == A.ZKE_OK, (ctx, key.name, int(got[i]["status"]), int(got[i]["detail"]))
                assert bytes(d_orc.em[i, :key.k]) == want


def expected_route(key):
    if key.e != 65537:
        return ROUTE_NOT_TAKEN
    return 4 if key.n.bit_length() <= 2048 else 8


def run_twice(eng, oracle, items, keys, ctx, routes2=None):
    """pass 1 (the wave routine fills the cache) and pass 2 (the lane-group routine), EM equal in both"""
    emails = [it[0] for it in items]
    got1, exp, d1, d2 = run_both(eng, oracle, emails)
    check_pass(got1, exp, d1, d2, items, keys, ctx + " pass 1")
    got2, exp2, d3, d4 = run_both(eng, oracle, emails)
    check_pass(got2, exp2, d3, d4, items, keys, ctx + " pass 2")
    routes2 = routes2 or [expected_route(k) for k in keys]
    assert [int(x) for x in d3.rsa_route[:len(keys)]] == routes2, (ctx, [hex(int(x)) for x in d3.rsa_route[:len(keys)]])
    assert (d1.em[:len(keys)] == d3.em[:len(keys)]).all(), ctx
    return d1


def pipeline_key_sets():
    """every synthetic modulus of 512 bits or more and every real test key, split into sets whose members have distinct
    key-cache slots (moduli like 2^(k-1) + 1 share their low limbs); one fresh engine per set"""
    keys = [edge_key(t, n) for t, n in rc.moduli()] + [synth.load_keys()[nm] for nm in KEY_NAMES]
    sets = []
    for k in keys:
        for s in sets:
            if key_cache_slot(k.n) not in {key_cache_slot(x.n) for x in s}:
                s.append(k)
                break
        else:
            sets.append([k])
    return sets


def fresh_engine():
    import zkemail_rs_amd as z
    return z.Engine(rsa_lane_groups=2)


@pytest.mark.parametrize("set_index", range(len(pipeline_key_sets())))
def test_lane_group_routine_edge_signatures(oracle, set_index):
    """Pass 1: every key is new, route 0x200 (not cached) and the wave routine takes it; pass 2: route exactly 4 / 8.
    Records equal the oracle, EM equals s^65537 mod n for accepted signatures and is all zero for rejected ones (s >= n,
    b= a byte short or long), the same in both passes; valid signatures under the odd-size keys verify."""
    keyset = pipeline_key_sets()[set_index]
    rng = np.random.default_rng(100 + set_index)
    prng = random.Random(200 + set_index)
    items, keys = [], []
    for key in keyset:
        sigs = rc.signatures(key.n, prng)
        if not isinstance(key, EdgeKey):
            sigs = rc.small_result_signatures(key, prng) + sigs
        for it in edge_emails(rng, key, len(items), sigs):
            items.append(it)
            keys.append(key)
    eng = fresh_engine()
    try:
        d1 = run_twice(eng, oracle, items, keys, f"key set {set_index}")
        for i, k in enumerate(keys):
            assert int(d1.rsa_route[i]) == (ROUTE_NOT_CACHED if k.e == 65537 else ROUTE_NOT_TAKEN), (k.name, hex(int(d1.rsa_route[i])))
    finally:
        eng.close()


def test_lane_group_routine_cache_collisions(oracle):
    """n2 = n1 + c 2^64 (same length) and n3 (another length) share n1's low 64 bits, hence its cache slot: once n1 owns
    the slot they route 0x400 (the wave routine) in every later batch, and their EM stays right."""
    keys = synth.load_keys()
    k1 = keys["rsa2048_03"]
    prng = random.Random(5)
    n2 = k1.n + (prng.getrandbits(1900) << 64)
    while n2.bit_length() != k1.n.bit_length():
        n2 = k1.n + (prng.getrandbits(1900) << 64)
    n3 = (k1.n & ((1 << 64) - 1)) + (prng.getrandbits(3000) << 64) | (1 << 3071)
    k2, k3 = edge_key("collide-same-length", n2), edge_key("collide-3072", n3)
    assert key_cache_slot(k2.n) == key_cache_slot(k3.n) == key_cache_slot(k1.n)
    rng = np.random.default_rng(6)
    eng = fresh_engine()
    try:
        first = edge_emails(rng, k1, 0, rc.small_result_signatures(k1, prng))
        run_twice(eng, oracle, first, [k1] * len(first), "n1 alone")
        items, ks = [], []
        for key in (k1, k2, k3):
            for it in edge_emails(rng, key, len(items), [(v, t) for v, t in rc.signatures(key.n, prng) if t in ("n-1", "random", "c0", "reject-n")]):
                items.append(it)
                ks.append(key)
        routes = [4 if k is k1 else ROUTE_SLOT_TAKEN for k in ks]
        d1 = run_twice(eng, oracle, items, ks, "colliding keys", routes)
        assert [int(x) for x in d1.rsa_route[:len(ks)]] == routes
    finally:
        eng.close()


def test_lane_group_routine_partial_groups(oracle):
    """Batches of 1, 15, 17, 33 four-lane e-mails and of 1, 7, 9 eight-lane e-mails (groups of a wave left partly empty),
    then one batch that mixes both with e-mails the wave routine takes (an e = 3 key)."""
    keys = synth.load_keys()
    four, eight, e3 = [keys["rsa2048_03"], keys["rsa2047_00"]], [keys["rsa4096_03"], keys["rsa3071_00"]], keys["rsa2047e3_00"]
    rng = np.random.default_rng(8)
    prng = random.Random(8)
    pool = {}
    for key in four + eight + [e3]:
        pool[key.name] = [(it, key) for it in edge_emails(rng, key, 0, rc.small_result_signatures(key, prng) + rc.signatures(key.n, prng))]
    eng = fresh_engine()
    try:
        warm = [p for key in four + eight for p in pool[key.name][:2]]
        run_twice(eng, oracle, [p[0] for p in warm], [p[1] for p in warm], "warm-up")
        for size, ks in [(1, four), (15, four), (17, four), (33, four), (1, eight), (7, eight), (9, eight)]:
            cand = [p for k in ks for p in pool[k.name]]
            pick = [cand[(3 * j + size) % len(cand)] for j in range(size)]
            run_twice(eng, oracle, [p[0] for p in pick], [p[1] for p in pick], f"{size} x {rc.group_lanes(ks[0].n.bit_length())} lanes")
        mixed = []
        for j in range(40):
            src = pool[(four + eight + [e3])[j % 5].name]
            mixed.append(src[j % len(src)])
        run_twice(eng, oracle, [p[0] for p in mixed], [p[1] for p in mixed], "mixed with the wave routine")
    finally:
        eng.close()
