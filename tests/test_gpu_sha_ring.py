"""GPU (-m gpu): the SHA-256 ring routine (csrc/sha256.hip.h sha256_ring_group) — a feeder wave and a rounds wave, two K+W
buffers, one barrier per block, the rounds wave reading its words while it runs the rounds — against hashlib and the CPU oracle,
beside the pair routine on the same inputs.

Engines: ZKE_SHA_RING = 1 and = 0 in the environment at creation (read once, there), and engines left to choose under
GPU_MAX_HW_QUEUES = 4 and = 8.  Block level through Engine.sha256_batch (sha256_ring_kernel / sha256_pair_kernel: group g =
messages 64 g .. 64 g + 63 in order); pipeline level through verify batches, where the routine runs inside the hash / modexp
launch with the length-bucketed job mapping, beside groups with a SHA-1 job (which the ring hands to the pair routine's one-wave
path) and groups without any job.  The lengths are those of tests/test_gpu_sha_handover.py, the block counts go on to 13: with
two buffers every block count up to there ends in either buffer after several turns, and every tile boundary (T = 128: a commit
every second block) is crossed."""
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

KNOBS = ("ZKE_SHA_RING", "GPU_MAX_HW_QUEUES")


def engine_with(env, **options):
    """an engine created with `env` in the environment (None: the variable unset), the environment restored afterwards"""
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
    """(forced ring, forced pair, chosen under 4 queues, chosen under 8 queues with 8 slots)"""
    queues = os.environ.get("GPU_MAX_HW_QUEUES")
    es = [engine_with({"ZKE_SHA_RING": 1, "GPU_MAX_HW_QUEUES": queues}), engine_with({"ZKE_SHA_RING": 0, "GPU_MAX_HW_QUEUES": queues}),
          engine_with({"GPU_MAX_HW_QUEUES": 4}, slots=8), engine_with({"GPU_MAX_HW_QUEUES": 8}, slots=8)]
    yield es
    for e in es:
        e.close()


def test_chosen_routine(engines):
    """Forced either way; by default min(slots that exist, GPU_MAX_HW_QUEUES at creation) <= 4 takes the ring: 8 slots under 4
    queues do, 8 slots under 8 queues do not, one slot under 8 queues does until zke_engine_reserve has grown it to 8."""
    ring, pair, q4, q8 = engines
    assert ring.sha_ring() and not pair.sha_ring() and q4.sha_ring() and not q8.sha_ring()
    eng = engine_with({"GPU_MAX_HW_QUEUES": 8})
    try:
        assert eng.sha_ring()
        eng.reserve(64, 1 << 20, 8)
        assert not eng.sha_ring()
    finally:
        eng.close()


@pytest.mark.parametrize("max_nblk", range(1, 14))
def test_one_long_lane(engines, max_nblk):
    """The group runs max_nblk steps while 63 lanes finished after the first; the long lane first, in the middle and last; a
    second group of the other parity rides in the same launch."""
    rng = np.random.default_rng(300 + max_nblk)
    long_len = 64 * max_nblk - 9
    assert nblk(long_len) == max_nblk and nblk(long_len + 1) == max_nblk + 1
    for pos in (0, 31, 63):
        group = [msg(rng, int(rng.integers(0, 56))) for _ in range(64)]
        group[pos] = msg(rng, long_len)
        other = [msg(rng, 64 * (max_nblk + 1) - 9 if i == 5 else 3) for i in range(64)]
        for eng in engines:
            check_digests(eng, group + other, f"max_nblk {max_nblk}, long lane {pos}, ring {eng.sha_ring()}")


@pytest.mark.parametrize("groups", [1, 2, 3])
def test_every_length_in_every_lane_position(engines, groups):
    """Lanes take the lengths of EDGE_LENS + BLOCKS_3_4_5 in turn (every group mixes 1 .. 5 blocks); the last group a single
    message, then filled up."""
    rng = np.random.default_rng(40 + groups)
    lens = EDGE_LENS + BLOCKS_3_4_5
    msgs = [msg(rng, lens[(i + i // 64) % len(lens)]) for i in range(64 * (groups - 1) + 1)]
    full = msgs + [msg(rng, lens[(3 * i) % len(lens)]) for i in range(63)]
    for eng in engines:
        check_digests(eng, msgs, f"{groups} groups, last one a single message, ring {eng.sha_ring()}")
        check_digests(eng, full, f"{groups} full groups, ring {eng.sha_ring()}")


def test_groups_of_one_length_each_and_the_empty_message(engines):
    rng = np.random.default_rng(47)
    msgs = [msg(rng, length) for length in EDGE_LENS + BLOCKS_3_4_5 for _ in range(64)]       # one group per length, one launch
    for eng in engines:
        check_digests(eng, msgs, f"groups of 64 equal lengths, ring {eng.sha_ring()}")
        assert bytes(eng.sha256_batch([b""])[0]) == hashlib.sha256(b"").digest()


def test_verify_batches_ragged_sha1_and_no_jobs(engines, oracle):
    """Through the hash / modexp launch of the forced-ring engine, then of the one that chose it: 64 ragged e-mails (length
    buckets, groups of different step counts in one launch), every fourth e-mail signed rsa-sha1 (those groups leave the ring for
    the one-wave path, their neighbours stay), three e-mails (groups of three jobs and groups of none), a batch in which nothing
    parses, and the ragged batch again."""
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
        assert eng.sha_ring()
        check_batch(eng, oracle, rag.emails, rag.inter, "ragged, 64 e-mails")
        check_batch(eng, oracle, emails, inter, "rsa-sha256 beside rsa-sha1")
        check_batch(eng, oracle, rag.emails[:3], rag.inter[:3], "three e-mails")
        got = eng.verify_batch(junk_batch)
        assert_records_equal(got, junk_exp, None, "nothing parses")
        assert all(int(s) != A.ZKE_OK for s in got["status"])
        check_batch(eng, oracle, rag.emails, rag.inter, "ragged again, behind the empty batch")
