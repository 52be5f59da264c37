"""GPU (-m gpu): the lane-group RSA routine on eight lanes of nine limbs (rsa_quad.hip.h rsa_group_wave<8, 9>: moduli of up to
2048 bits, in place of four lanes of eighteen), against Python's pow(s, 65537, n), the oracle's records and the four-lane routine.

Reached the way tests/test_gpu_rsa_edges.py reaches the lane groups — through the pipeline of an engine with rsa_lane_groups = 2,
every batch twice: the first pass takes the one-signature-per-wave routine, which fills the key cache, the second finds the keys
cached — with the role forced by ZKE_RSA_OCT9 in the environment at engine creation (1: route 16 = RSA_F_OCT9; 0: route 4, the
four-lane role, whose records and EM bytes on the same batch must be identical).  A wave holds 8 signatures and a workgroup two
waves: 1 / 7 / 8 / 9 / 17 signatures are a partial wave, one short of a wave, a full wave, one more, and two workgroups with a
ragged tail.  tests/test_rsa_oct9_model.py is the CPU model of the arithmetic and of the EMSA limb classes; a non-zero byte at or
above k, which a reduced EM (< n < 2^(8k)) cannot hold on the device, is covered there only (the zero-limb class for every k) —
here the nearest case is a non-zero top byte inside k.

The last test leaves the role to the engine: min(slots that exist, GPU_MAX_HW_QUEUES as read at creation) <= 4 takes eight lanes."""
import os
import random

import numpy as np
import pytest

import synth
from test_gpu_rsa_edges import check_pass, edge_emails, key_cache_slot, make_email
from test_gpu_verify import assert_records_equal, run_both
from zkemail_rs_amd import _abi as A

pytestmark = pytest.mark.gpu

ROUTE_OCT9, ROUTE_QUAD, ROUTE_OCT = 16, 4, 8
SIZES = (1, 7, 8, 9, 17)


def is_prime(x, rng):
    if x % 2 == 0:
        return x == 2
    d, s = x - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for _ in range(24):
        y = pow(rng.randrange(2, x - 1), d, x)
        if y in (1, x - 1):
            continue
        for _ in range(s - 1):
            y = y * y % x
            if y == x - 1:
                break
        else:
            return False
    return True


def make_key(bits, seed):
    """a real key of a size tests/golden/keys.json does not hold (512 bits: the smallest the lane groups take)"""
    rng = random.Random(seed)

    def prime(b):
        while True:
            x = rng.getrandbits(b) | (3 << (b - 2)) | 1
            if x % 65537 != 1 and is_prime(x, rng):
                return x
    p, q = prime(bits // 2), prime(bits - bits // 2)
    n = p * q
    assert n.bit_length() == bits and p != q
    d = pow(65537, -1, (p - 1) * (q - 1))
    return synth.RsaKey(f"rsa{bits}_made", bits, n, 65537, d, p, q, synth.pkcs1_pub_der(n, 65537))


def keys_under_test():
    ks = synth.load_keys()
    return {512: make_key(512, 512), 1024: ks["rsa1024_00"], 2047: ks["rsa2047_00"], 2048: ks["rsa2048_03"]}


def forced_engine(oct9):
    import zkemail_rs_amd as z
    old = os.environ.get("ZKE_RSA_OCT9")
    os.environ["ZKE_RSA_OCT9"] = "1" if oct9 else "0"              # read once, at engine creation
    try:
        return z.Engine(rsa_lane_groups=2)
    finally:
        if old is None:
            del os.environ["ZKE_RSA_OCT9"]
        else:
            os.environ["ZKE_RSA_OCT9"] = old


@pytest.fixture(scope="module")
def engines():
    e9, e4 = forced_engine(True), forced_engine(False)
    yield e9, e4
    e9.close()
    e4.close()


def bad_emsa_signatures(key, em):
    """-> [(s, tag)]: signatures whose EM (the well-formed `em` of this e-mail, altered) has no EMSA shape; s = EM'^d mod n."""
    k = key.k
    tlen = 51
    out = []

    def put(pos, byte, tag):                                          # big-endian byte index
        bad = em[:pos] + bytes([byte]) + em[pos + 1:]
        assert bad != em and int.from_bytes(bad, "big") < key.n
        out.append((pow(int.from_bytes(bad, "big"), key.d, key.n), tag))
    put(k - tlen - 2, 0x00, "ff-run-a-byte-short")                   # 00 one byte early: the run is short (and the separator doubled)
    put(2 + (k - tlen - 3) // 2, 0x00, "ff-run-broken-in-the-middle")
    put(2, 0xFE, "ff-run-first-byte")
    put(k - tlen + 3, em[k - tlen + 3] ^ 0x04, "digestinfo")         # inside the DigestInfo prefix
    put(k - 33, 0x21, "digestinfo-length-byte")                      # its last byte (the digest length)
    put(1, 0x02, "block-type")
    if key.n >> (8 * k - 8) > 1:                                      # the top byte: EM < n lets it be non-zero only under such a modulus.  (A reduced
        put(0, 0x01, "nonzero-top-byte")                              # EM has no byte at or above k at all; this is the highest one there is.)
    return out


def pool_for(key, rng, prng):
    """17 e-mails under one key: the operand edges (s = 0, 1, n - 1, s = n, s > n, b= a byte short / long), EM without EMSA shape,
    valid signatures, random ones to fill up"""
    n = key.n
    sigs = [(0, "zero"), (1, "one"), (n - 1, "n-1"), (n, "reject-n")]
    if n + 2 < 1 << (8 * key.k):
        sigs.append((n + 2, "reject-above-n"))
    sigs.append(((1 << (8 * key.k)) - 1, "reject-all-ones"))
    items = edge_emails(rng, key, 0, sigs)                            # + "short", "long", "valid"
    probe, em = make_email(rng, len(items), key)
    for s, tag in bad_emsa_signatures(key, em):
        items.append(make_email(rng, len(items), key, s.to_bytes(key.k, "big")) + (tag,))
    items.append((probe, em, "valid"))
    while len(items) < max(SIZES):
        items.append(make_email(rng, len(items), key, prng.randrange(n).to_bytes(key.k, "big")) + ("random",))
    return items[:max(SIZES)]


def run_pair(engines, oracle, items, keys, ctx, routes9):
    """the batch twice on the forced eight-lane engine and twice on the forced four-lane one; second passes compared"""
    e9, e4 = engines
    emails = [it[0] for it in items]
    second = []
    for eng, name in ((e9, "oct9"), (e4, "quad")):
        for npass in (1, 2):
            got, exp, d_gpu, d_orc = run_both(eng, oracle, emails)
            check_pass(got, exp, d_gpu, d_orc, items, keys, f"{ctx} {name} pass {npass}")
        second.append((got, d_gpu))
    (got9, d9), (got4, d4) = second
    routes4 = [ROUTE_QUAD if r == ROUTE_OCT9 else r for r in routes9]
    assert [int(x) for x in d9.rsa_route[:len(keys)]] == routes9, (ctx, [hex(int(x)) for x in d9.rsa_route[:len(keys)]])
    assert [int(x) for x in d4.rsa_route[:len(keys)]] == routes4, (ctx, [hex(int(x)) for x in d4.rsa_route[:len(keys)]])
    assert_records_equal(got9, got4, None, ctx + " eight lanes against four")
    assert (d9.em[:len(keys)] == d4.em[:len(keys)]).all(), ctx


@pytest.mark.parametrize("bits", [512, 1024, 2047, 2048])
def test_oct9_operands_emsa_and_fill(engines, oracle, bits):
    key = keys_under_test()[bits]
    assert key.n.bit_length() == bits
    rng, prng = np.random.default_rng(9000 + bits), random.Random(9000 + bits)
    pool = pool_for(key, rng, prng)
    tags = [it[2] for it in pool]
    assert {"zero", "one", "n-1", "reject-n", "short", "long", "valid", "ff-run-a-byte-short", "digestinfo", "block-type"} <= set(tags)
    for size in SIZES:
        pick = pool if size == len(pool) else [pool[(5 * j + size) % len(pool)] for j in range(size)]
        run_pair(engines, oracle, pick, [key] * size, f"{bits} bits x {size}", [ROUTE_OCT9] * size)
    # the EMSA failures are failures, the valid ones verify (check_pass has compared every record with the oracle's)
    got, _, _, _ = run_both(engines[0], oracle, [it[0] for it in pool])
    for r, tag in zip(got, tags):
        assert (int(r["status"]) == A.ZKE_OK) == (tag == "valid"), tag
        if tag != "valid":
            assert int(r["status"]) == A.ZKE_DKIM_NOT_PASS and int(r["detail"]) == A.D_SIG_MISMATCH, tag


def test_oct9_shares_a_launch_with_eight_lanes_of_eighteen(engines, oracle):
    """<= 2048-bit and 4096-bit keys in one batch: routes 16 and 8 in one launch (the four-lane engine: 4 and 8)."""
    ks = synth.load_keys()
    small, big = [keys_under_test()[2048], ks["rsa1024_00"], keys_under_test()[2047]], [ks["rsa4096_03"], ks["rsa3071_00"]]
    slots = [key_cache_slot(k.n) for k in small + big + [keys_under_test()[512]]]
    assert len(set(slots)) == len(slots)                              # the module's engines hold every key of this file at once
    rng, prng = np.random.default_rng(96), random.Random(96)
    items, keys = [], []
    for j in range(21):
        key = (small + big)[j % 5]
        sig = None if j % 3 else prng.randrange(key.n).to_bytes(key.k, "big")
        items.append(make_email(rng, j, key, sig) + ("valid" if sig is None else "random",))
        keys.append(key)
    assert sum(len(k.pkcs1_der) for k in keys) > 272 * len(keys)      # the batch's keys average above an RSA-2048 key: the <8, 18> role joins
    routes = [ROUTE_OCT9 if k.n.bit_length() <= 2048 else ROUTE_OCT for k in keys]
    run_pair(engines, oracle, items, keys, "mixed sizes", routes)


def engine_under_queue_cap(cap, **options):
    """an engine that reads GPU_MAX_HW_QUEUES = cap at its creation and no forced role (the variable only sizes HIP's pool when the
    runtime starts; what is tested is the engine's own reading of it)"""
    import zkemail_rs_amd as z
    old = {k: os.environ.get(k) for k in ("GPU_MAX_HW_QUEUES", "ZKE_RSA_OCT9")}
    os.environ["GPU_MAX_HW_QUEUES"] = str(cap)
    os.environ.pop("ZKE_RSA_OCT9", None)
    try:
        return z.Engine(**options)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_default_choice_of_the_role():
    """No forced role, rsa_lane_groups = 0, a batch of 256 e-mails (the size from which the lane groups join): an engine created
    with 22 slots under a cap of 23 queues routes 4; one with default options (one slot) routes 16; that one grown to 22 slots by
    zke_engine_reserve routes 4 from then on; and 22 slots under a cap of 4 queues route 16.  Every batch verifies."""
    wl = synth.make_workload("oct9-default", 256, 300, rsa_bits=2048, n_keys=2, seed=909)
    batch = A.PackedBatch(wl.emails)
    mx = max(len(e.raw_email) for e in wl.emails)
    raw_total = sum(len(e.raw_email) for e in wl.emails)

    def routes(eng):
        eng.verify_batch(batch)                                       # the keys are cached behind this one
        dbg = A.DebugBuffers(batch.n, 2 * mx + 4096, mx + 64)
        got = eng.verify_batch(batch, dbg)
        assert (np.asarray(got["status"]) == A.ZKE_OK).all()
        return {int(x) for x in dbg.rsa_route[:batch.n]}

    eng = engine_under_queue_cap(23, slots=22)
    try:
        assert routes(eng) == {ROUTE_QUAD}
    finally:
        eng.close()
    eng = engine_under_queue_cap(23)
    try:
        assert routes(eng) == {ROUTE_OCT9}
        eng.reserve(batch.n, raw_total + 64, 22)
        assert routes(eng) == {ROUTE_QUAD}
    finally:
        eng.close()
    eng = engine_under_queue_cap(4, slots=22)
    try:
        assert routes(eng) == {ROUTE_OCT9}
    finally:
        eng.close()
