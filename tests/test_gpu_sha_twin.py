"""GPU (-m gpu): the SHA-256 twin routine (csrc/sha256.hip.h sha256_twin_group) — the ring with groups of 32 messages, two lanes
per message in the rounds wave (e..h in one, a..d in its partner, exchanged by DPP), two blocks per feeder pass and one barrier
per pass — against hashlib and the CPU oracle, beside the one-lane ring on the same inputs.

Engines: the twin forced (ZKE_SHA_RING = 1, ZKE_SHA_TWIN = 1), the ring with the twin forced off (ZKE_SHA_TWIN = 0: the one-lane
ring stays covered, since an engine left to choose now takes the twin wherever it takes the ring), and engines left to choose
under GPU_MAX_HW_QUEUES = 4 and = 8 with 8 slots.  Block level through Engine.sha256_batch (sha256_twin_kernel: group g =
messages 32 g .. 32 g + 31 in order, message p in lanes 8 (p / 4) + p % 4 and 8 (p / 4) + 7 - p % 4 of the rounds wave, in lanes
p and p + 32 of the feeder); pipeline level through verify batches, where bodies and header preimages take twin groups under the
length buckets, domains and keys ring groups, and a group with a SHA-1 job the one-wave path."""
import hashlib
import os

import numpy as np
import pytest

import synth
from test_gpu_sha_edges import check_batch, check_digests
from test_gpu_sha_handover import BLOCKS_3_4_5, EDGE_LENS, msg, nblk
from test_gpu_verify import assert_records_equal
from zkemail_rs_amd import _abi as A

pytestmark = pytest.mark.gpu

KNOBS = ("ZKE_SHA_RING", "ZKE_SHA_TWIN", "GPU_MAX_HW_QUEUES")


def engine_with(env, **options):
    """an engine created with `env` in the environment (None or missing: the variable unset), the environment restored afterwards"""
    import zkemail_rs_amd as z
    old = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        v = env.get(k)
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        return z.Engine(**options)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def engines():
    """(forced twin, ring without the twin, chosen under 4 queues, chosen under 8 queues with 8 slots)"""
    queues = os.environ.get("GPU_MAX_HW_QUEUES")
    es = [engine_with({"ZKE_SHA_RING": 1, "ZKE_SHA_TWIN": 1, "GPU_MAX_HW_QUEUES": queues}),
          engine_with({"ZKE_SHA_RING": 1, "ZKE_SHA_TWIN": 0, "GPU_MAX_HW_QUEUES": queues}),
          engine_with({"GPU_MAX_HW_QUEUES": 4}, slots=8), engine_with({"GPU_MAX_HW_QUEUES": 8}, slots=8)]
    yield es
    for e in es:
        e.close()


def tag(eng):
    return f"ring {eng.sha_ring()}, twin {eng.sha_twin()}"


def test_chosen_mapping(engines):
    """The twin is taken wherever the ring is, unless ZKE_SHA_TWIN = 0; where the pair is taken, ZKE_SHA_TWIN = 1 changes nothing."""
    twin, ring, q4, q8 = engines
    assert twin.sha_ring() and twin.sha_twin()
    assert ring.sha_ring() and not ring.sha_twin()
    assert q4.sha_ring() and q4.sha_twin()
    assert not q8.sha_ring() and not q8.sha_twin()
    eng = engine_with({"ZKE_SHA_RING": 0, "ZKE_SHA_TWIN": 1})
    try:
        assert not eng.sha_ring() and not eng.sha_twin()
    finally:
        eng.close()


@pytest.mark.parametrize("count", [1, 31, 32, 33, 63, 64, 65, 97])
def test_message_counts(engines, count):
    """A last group of one message, a full group, a group boundary at 32; lengths of 1 .. 5 blocks in turn."""
    rng = np.random.default_rng(500 + count)
    lens = EDGE_LENS + BLOCKS_3_4_5
    msgs = [msg(rng, lens[(5 * i + count) % len(lens)]) for i in range(count)]
    for eng in engines:
        check_digests(eng, msgs, f"{count} messages, {tag(eng)}")


@pytest.mark.parametrize("max_nblk", range(1, 14))
def test_one_long_message(engines, max_nblk):
    """The group runs max_nblk steps — odd: the upper feeder lanes idle in the last pass, and the rounds wave meets the last
    barrier behind an even block — while 31 messages finished after the first; the long one at pair positions 0, 15 and 31; a
    second group of the other parity rides in the same launch."""
    rng = np.random.default_rng(600 + max_nblk)
    long_len = 64 * max_nblk - 9
    assert nblk(long_len) == max_nblk and nblk(long_len + 1) == max_nblk + 1
    for pos in (0, 15, 31):
        group = [msg(rng, int(rng.integers(0, 56))) for _ in range(32)]
        group[pos] = msg(rng, long_len)
        other = [msg(rng, 64 * (max_nblk + 1) - 9 if i == 5 else 3) for i in range(32)]
        for eng in engines:
            check_digests(eng, group + other, f"max_nblk {max_nblk}, long message at {pos}, {tag(eng)}")


def test_every_length_in_every_lane_position(engines):
    """Every length of EDGE_LENS + BLOCKS_3_4_5 at every position of a group: 15 groups, each the lengths shifted by one."""
    rng = np.random.default_rng(71)
    lens = EDGE_LENS + BLOCKS_3_4_5
    msgs = [msg(rng, lens[(p + g) % len(lens)]) for g in range(len(lens)) for p in range(32)]
    for eng in engines:
        check_digests(eng, msgs, f"every length at every position, {tag(eng)}")


def test_groups_of_one_length_each_and_the_empty_message(engines):
    rng = np.random.default_rng(72)
    msgs = [msg(rng, length) for length in EDGE_LENS + BLOCKS_3_4_5 for _ in range(32)]       # one twin group per length, one launch
    for eng in engines:
        check_digests(eng, msgs, f"groups of 32 equal lengths, {tag(eng)}")
        assert bytes(eng.sha256_batch([b""])[0]) == hashlib.sha256(b"").digest()


def test_verify_batches_ragged_sha1_and_no_jobs(engines, oracle):
    """The sequence of tests/test_gpu_sha_ring.py through the hash / modexp launch of the forced-twin engine, then of the one that
    chose it: 64 ragged e-mails, every fourth e-mail signed rsa-sha1 (those groups leave for the one-wave path, 32 wide), three
    e-mails, a batch in which nothing parses, and the ragged batch again."""
    rag = synth.make_workload("ring-ragged", 64, 20000, n_keys=4, seed=33, ragged=True, invalid_frac=0.05)
    s1 = synth.make_workload("ring-sha1", 16, 3000, n_keys=4, seed=34, ragged=True, algo="rsa-sha1")
    emails, inter = [], []
    for k in range(16):
        emails += rag.emails[3 * k:3 * k + 3] + [s1.emails[k]]
        inter += rag.inter[3 * k:3 * k + 3] + [s1.inter[k]]
    junk = [A.Email("example.com", b"no header block, no signature" * (i + 1), rag.emails[0].public_key) for i in range(5)]
    junk_batch = A.PackedBatch(junk)
    junk_exp = oracle.verify_batch(junk_batch, threads=2)
    for eng in (engines[0], engines[2]):
        assert eng.sha_twin()
        check_batch(eng, oracle, rag.emails, rag.inter, "ragged, 64 e-mails")
        check_batch(eng, oracle, emails, inter, "rsa-sha256 beside rsa-sha1")
        check_batch(eng, oracle, rag.emails[:3], rag.inter[:3], "three e-mails")
        got = eng.verify_batch(junk_batch)
        assert_records_equal(got, junk_exp, None, "nothing parses")
        assert all(int(s) != A.ZKE_OK for s in got["status"])
        check_batch(eng, oracle, rag.emails, rag.inter, "ragged again, behind the empty batch")


def test_verify_batch_of_96_ragged(engines, oracle):
    """96 e-mails, 5 % of them corrupted on purpose: a kind's job list is padded beyond them, so under the buckets its twin groups
    are full ones, a partly filled one wherever an e-mail brings no message of the kind, and groups with nothing to do."""
    rag = synth.make_workload("twin-ragged-96", 96, 6000, n_keys=4, seed=35, ragged=True, invalid_frac=0.05)
    for eng in (engines[0], engines[2]):
        check_batch(eng, oracle, rag.emails, rag.inter, f"ragged, 96 e-mails, {tag(eng)}")
