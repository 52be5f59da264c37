"""GPU (-m gpu): the lane-group RSA routine (rsa_quad.hip.h rsa_group_wave<4> / <8>) at 18 limbs of 29 bits per lane,
on the operands that layout can get wrong, against Python's pow(s, 65537, n) and the oracle's records.

The routine is reached the way tests/test_gpu_rsa_edges.py reaches it: through the pipeline of an engine with
rsa_lane_groups = 2, every batch twice — the first pass takes the one-signature-per-wave routine, whose pre-pass fills the
key cache (R'^2 mod n as 29-bit limbs, KeyCacheEntry::rrq), the second pass is routed to four lanes per signature
(512..2048 bits) or eight (..4096), asserted from the route the front end reports.  (The building-block entry
zke_rsa_modexp_batch runs without a key cache, so it never reaches the lane groups; the whole EM comes from the
pipeline's debug buffers instead.)  tests/rsa_edge_cases.py aims its lane-boundary values at the former 532 bits per
lane; the boundaries here are the 522-bit ones of tests/test_rsa_group_model29.py."""
import os
import random
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import synth
from test_gpu_rsa_edges import (ROUTE_SLOT_TAKEN, edge_emails, edge_key, fresh_engine, key_cache_slot, make_email, run_twice)

pytestmark = pytest.mark.gpu

QL, QBITS = 18, 29
MASK = (1 << QBITS) - 1
LANE_BITS = QL * QBITS                                   # 522
BIG_KEY_HINT = 272                                       # bytes of key per e-mail above which a batch gets the eight-lane role


class Engines:
    """Engines of the module, made on demand.  A key cache slot holds one modulus for an engine's life and the shaped
    moduli below share their low 64 bits (all ones; the alternating pattern), hence their slot: a key goes to the first
    engine whose slot is still free or already its own."""

    def __init__(self):
        self.engines, self.slots = [], []

    def of(self, key):
        slot = key_cache_slot(key.n)
        for eng, taken in zip(self.engines, self.slots):
            if taken.setdefault(slot, key.n) == key.n:
                return eng
        self.engines.append(fresh_engine())
        self.slots.append({slot: key.n})
        return self.engines[-1]

    def close(self):
        for eng in self.engines:
            eng.close()


@pytest.fixture(scope="module")
def engines():
    e = Engines()
    yield e
    e.close()


def rand_odd(bits, rng):
    return rng.getrandbits(bits) | (1 << (bits - 1)) | 1


def alternating(bits, first):
    """limbs equal to 2^29 - 1 next to limbs equal to 0, starting with `first` (0 / 1) at limb 0, cut to `bits` bits"""
    x = sum(MASK << (QBITS * t) for t in range(first ^ 1, bits // QBITS + 2, 2))
    return x & ((1 << bits) - 1)


def limb_signatures(n, rng):
    """-> [(s, tag)]: 0, 1, n-1, n-2; s and n differing only in lane p (n -+ 2^(522 p): accepted / rejected by that lane
    alone); values around a lane boundary; alternating full / empty limbs; s = n."""
    bits = n.bit_length()
    G = 4 if bits <= 2048 else 8
    out = [(0, "zero"), (1, "one"), (n - 2, "n-2"), (n - 1, "n-1"), (rng.randrange(n), "random"), (n, "reject-n")]
    for p in range(G):
        d = 1 << (LANE_BITS * p)
        if d < n:
            out += [(n - d, f"n-lane{p}"), (n + d, f"reject-lane{p}"), (d - 1, f"below-lane{p}"), (d + 1, f"above-lane{p}")]
    out += [(alternating(bits, 1), "alt-ones-first"), (alternating(bits, 0), "alt-zero-first"),
            (alternating(bits - 1, 1), "alt-short")]
    seen, uniq = set(), []
    for s, t in out:
        if s >= 0 and s not in seen:                               # (values at or above n are rejected: EM stays all zero)
            seen.add(s)
            uniq.append((s, t))
    return uniq


def shaped_modulus(tag, bits):
    if tag == "ones":
        return (1 << bits) - 1
    if tag == "smallest":
        return (1 << (bits - 1)) + 1
    if tag == "alt":
        return alternating(bits, 1) | (1 << (bits - 1))             # odd: limb 0 is all ones
    if tag.startswith("lane"):                                      # 2^k - 2^(522 p) - 1: ones, a hole at the boundary, ones
        return (1 << bits) - (1 << (LANE_BITS * int(tag[4:]))) - 1
    return rand_odd(bits, random.Random(bits))


MODULI = [("random", b) for b in (1024, 1537, 2048, 2049, 3072, 4096)] + \
         [("ones", 2048), ("ones", 4096), ("alt", 2048), ("alt", 4096), ("smallest", 2048), ("lane2", 2048), ("lane5", 4096)]


@pytest.mark.parametrize("tag,bits", MODULI, ids=[f"{t}{b}" for t, b in MODULI])
def test_limb_layout_edge_operands(engines, oracle, tag, bits):
    """Pass 2 is routed to four / eight lanes; EM equals pow(s, 65537, n) for accepted signatures and is all zero for
    rejected ones (s >= n decided by one lane, b= a byte short or long), records equal the oracle's."""
    n = shaped_modulus(tag, bits)
    assert n & 1 and n.bit_length() == bits
    key = edge_key(f"{tag}{bits}", n)
    eng = engines.of(key)
    rng, prng = np.random.default_rng(bits), random.Random(bits + 1)
    items = edge_emails(rng, key, 0, limb_signatures(n, prng))
    assert sum(1 for it in items if it[1] is not None) >= 8
    keys = [key] * len(items)
    if bits > 2048 and len(key.pkcs1_der) <= BIG_KEY_HINT:
        # The eight-lane role joins a launch only when the batch's keys average more than BIG_KEY_HINT bytes (pipeline.hip.h:
        # the hint that a batch holds keys above 2048 bits at all); a 2049-bit key's DER is 270.  Two e-mails under a 3071-bit
        # key lift the average, as any mixed batch does; they take the eight-lane route too.
        big = synth.load_keys()["rsa3071_00"]
        assert engines.of(big) is eng
        items += [make_email(rng, len(items) + i, big) + ("valid",) for i in range(2)]
        keys += [big, big]
        assert sum(len(k.pkcs1_der) for k in keys) > BIG_KEY_HINT * len(keys)
    run_twice(eng, oracle, items, keys, f"{tag}{bits}")


@pytest.mark.parametrize("name,fills", [("rsa2047_00", (1, 15, 16, 17)), ("rsa4095_00", (1, 7, 8, 9))])
def test_group_fill(engines, oracle, name, fills):
    """A wave holds 16 four-lane or 8 eight-lane signatures: one, one short of a wave, exactly a wave, one more."""
    key = synth.load_keys()[name]
    eng = engines.of(key)
    rng, prng = np.random.default_rng(29), random.Random(29)
    pool = [make_email(rng, i, key) + ("valid",) for i in range(3)]
    while len(pool) < max(fills):
        s = prng.randrange(key.n)
        pool.append(make_email(rng, len(pool), key, s.to_bytes(key.k, "big")) + ("random",))
    run_twice(eng, oracle, pool[:2], [key] * 2, f"{name} warm-up")
    for size in fills:
        pick = [pool[(j + size) % len(pool)] for j in range(size)]
        run_twice(eng, oracle, pick, [key] * size, f"{name} x {size}")


def test_two_keys_in_one_cache_slot(engines, oracle):
    """n2 shares n1's low 64 bits, hence its slot: n1 owns it and takes the lane groups, n2 keeps the wave routine (route
    0x400) and must never be served n1's constants; EM right for both, in one batch."""
    k1 = synth.load_keys()["rsa1024_00"]
    eng = engines.of(k1)
    prng = random.Random(290)
    n2 = k1.n + (prng.getrandbits(900) << 64)
    while n2.bit_length() != k1.n.bit_length():
        n2 = k1.n + (prng.getrandbits(900) << 64)
    k2 = edge_key("collides-with-rsa1024_00", n2)
    assert key_cache_slot(k2.n) == key_cache_slot(k1.n)
    rng = np.random.default_rng(291)
    first = [make_email(rng, 0, k1) + ("valid",)]
    run_twice(eng, oracle, first, [k1], "slot owner alone")
    items, ks = [], []
    for key in (k1, k2, k1, k2):
        for s, t in limb_signatures(key.n, prng)[:6]:
            if s < 1 << (8 * key.k):
                items.append(make_email(rng, len(items), key, s.to_bytes(key.k, "big")) + (t,))
                ks.append(key)
    routes = [4 if k is k1 else ROUTE_SLOT_TAKEN for k in ks]
    d1 = run_twice(eng, oracle, items, ks, "colliding keys", routes)
    assert [int(x) for x in d1.rsa_route[:len(ks)]] == routes


def test_whole_pipeline_device_entry():
    """33 e-mails over three keys (1024 / 2048 / 4096 bits), one signature corrupted, through zke_verify_batch_device three
    times (the first submission fills the key cache, the later ones run four and eight lanes per signature in one launch):
    every submission's records equal the oracle's.  (The device entry has no debug buffers, so the route is not read here: that
    a cached key of either size takes the lane groups in an engine with rsa_lane_groups = 2 is what the tests above assert from
    rsa_route; this one adds the mixed launch and the production entry.)  In a subprocess: torch owns the device buffers and has to initialise
    HIP before the engine does."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent(f"""
        import sys
        sys.path.insert(0, {root!r}); sys.path.insert(0, {os.path.join(root, 'tests')!r})
        import numpy as np, torch
        torch.zeros(1, device="cuda")
        import bench, oracle_lib, synth, zkemail_rs_amd as z
        from zkemail_rs_amd import _abi as A
        from test_gpu_verify import assert_records_equal
        from test_gpu_rsa_edges import make_email
        keys = [synth.load_keys()[k] for k in ("rsa1024_00", "rsa2048_03", "rsa4096_03")]
        rng = np.random.default_rng(33)
        emails = []
        for i in range(33):
            key = keys[i % 3]
            sig = None
            if i == 16:                      # a signature of another message: b= decodes, s < n, EM has no EMSA shape
                sig = pow(12345678901234567890, key.d, key.n).to_bytes(key.k, "big")
            emails.append(make_email(rng, i, key, sig)[0])
        packed = A.PackedBatch(emails)
        exp = oracle_lib.load().verify_batch(packed, threads=4)
        assert [int(s) for s in exp["status"]].count(A.ZKE_OK) == 32 and int(exp[16]["status"]) == A.ZKE_DKIM_NOT_PASS
        engine = z.Engine(0, rsa_lane_groups=2)
        dev = torch.device("cuda", 0)
        cb, keep, totals = bench.device_batch(torch, packed, dev)
        out = torch.zeros(packed.n * 192, dtype=torch.uint8, device=dev)
        st = torch.cuda.Stream()
        for rep in range(3):
            out.zero_()
            torch.cuda.synchronize()
            engine.verify_batch_device(cb, totals[0], totals[1], totals[2], out.data_ptr(), st.cuda_stream)
            torch.cuda.synchronize()
            assert_records_equal(out.cpu().numpy().view(A.RESULT_DTYPE), exp, None, f"submission {{rep}}")
        engine.close()
        print("limb29 device entry ok")
    """)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "limb29 device entry ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
