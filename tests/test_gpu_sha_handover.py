"""GPU (-m gpu): the block loop of the SHA-256 pair routine (csrc/sha256.hip.h sha256_pair_group) — a feeder wave and a rounds
wave that hand 64 K+W words per block over through one LDS buffer and meet at two barriers per block on every path — against
hashlib and the CPU oracle, at the block counts and group shapes where the two waves' barrier counts or a lane that ends early
could go wrong: max_nblk 1, odd and even, one lane at the maximum and the rest at one block, lanes without a job, groups without
any.

Block level: Engine.sha256_batch (zke_sha256_batch: the body of zke_sha256_batch_device between two copies; up to 512 groups of 64
messages it launches sha256_pair_kernel, group g = messages 64 g .. 64 g + 63 in order).  Pipeline level: verify batches, where the
routine runs inside hash_modexp_kernel with the length-bucketed job mapping, beside groups with a SHA-1 job (the one-wave path) and
groups without any job.  tests/test_gpu_sha_edges.py sweeps the padding edges at size; this file keeps to the loop structure."""
import hashlib

import numpy as np
import pytest

import synth
from test_gpu_sha_edges import check_batch, check_digests
from test_gpu_verify import assert_records_equal
from zkemail_rs_amd import _abi as A

pytestmark = pytest.mark.gpu

EDGE_LENS = (0, 55, 56, 63, 64, 119, 120, 127, 128)                   # one and two blocks, both sides of every padding edge
BLOCKS_3_4_5 = (129, 183, 184, 247, 248, 311)                         # 3, 3, 4, 4, 5, 5 blocks


def nblk(length):
    return (length + 9 + 63) // 64


def msg(rng, length):
    return rng.integers(0, 256, length, dtype=np.uint8).tobytes()


def test_block_counts_of_the_edge_lengths():
    assert [nblk(x) for x in EDGE_LENS] == [1, 1, 2, 2, 2, 2, 3, 3, 3] and [nblk(x) for x in BLOCKS_3_4_5] == [3, 3, 4, 4, 5, 5]


@pytest.mark.parametrize("groups", [1, 2, 3])
def test_every_length_in_every_lane_position(engine, groups):
    """1, 2 and 3 groups whose lanes take the lengths in turn (so every group mixes 1 .. 5 blocks and lanes end at different
    blocks), the last group cut to a single message: its other 63 lanes have no job at all."""
    rng = np.random.default_rng(groups)
    lens = EDGE_LENS + BLOCKS_3_4_5
    msgs = [msg(rng, lens[(i + i // 64) % len(lens)]) for i in range(64 * (groups - 1) + 1)]
    check_digests(engine, msgs, f"{groups} groups, last one a single message")
    msgs += [msg(rng, lens[(3 * i) % len(lens)]) for i in range(63)]
    check_digests(engine, msgs, f"{groups} full groups")


@pytest.mark.parametrize("max_nblk", [1, 2, 3, 4, 5, 6, 7, 9])
def test_one_lane_at_the_maximum_the_rest_at_one_block(engine, max_nblk):
    """The group runs max_nblk steps, odd and even counts, while 63 lanes finished after the first; the long lane sits first, last
    and in the middle, and a second group of another parity rides in the same launch."""
    rng = np.random.default_rng(100 + max_nblk)
    long_len = 64 * max_nblk - 9                                      # exactly max_nblk blocks, the length field in the last one
    assert nblk(long_len) == max_nblk and nblk(long_len + 1) == max_nblk + 1
    for pos in (0, 31, 63):
        group = [msg(rng, int(rng.integers(0, 56))) for _ in range(64)]
        group[pos] = msg(rng, long_len)
        other = [msg(rng, 64 * (max_nblk + 1) - 9 if i == 5 else 3) for i in range(64)]
        check_digests(engine, group + other, f"max_nblk {max_nblk}, long lane {pos}")


def test_groups_of_one_length_each(engine):
    """All 64 lanes alike, one group per length: empty messages (one block of padding only) up to five blocks."""
    rng = np.random.default_rng(7)
    for length in EDGE_LENS + BLOCKS_3_4_5:
        check_digests(engine, [msg(rng, length) for _ in range(64)], f"64 messages of {length} bytes")


def test_verify_batches_ragged_sha1_and_no_jobs(engine, oracle):
    """Through hash_modexp_kernel: 64 e-mails with ragged bodies (length buckets: lanes of a group within an eighth of each other,
    groups of different step counts in one launch), the same with every fourth e-mail signed rsa-sha1 (those groups take the
    one-wave path, their neighbours the pair loop), three e-mails (groups of three jobs and groups of none), and a batch none of
    whose e-mails parses: every SHA group of its launch is padding jobs only."""
    rag = synth.make_workload("handover-ragged", 64, 20000, n_keys=4, seed=31, ragged=True, invalid_frac=0.05)
    check_batch(engine, oracle, rag.emails, rag.inter, "ragged, 64 e-mails")
    s1 = synth.make_workload("handover-sha1", 16, 3000, n_keys=4, seed=32, ragged=True, algo="rsa-sha1")
    emails, inter = [], []
    for k in range(16):
        emails += rag.emails[3 * k:3 * k + 3] + [s1.emails[k]]
        inter += rag.inter[3 * k:3 * k + 3] + [s1.inter[k]]
    check_batch(engine, oracle, emails, inter, "rsa-sha256 beside rsa-sha1")
    check_batch(engine, oracle, rag.emails[:3], rag.inter[:3], "three e-mails")
    junk = [A.Email("example.com", b"no header block, no signature" * (i + 1), rag.emails[0].public_key) for i in range(5)]
    batch = A.PackedBatch(junk)
    got, exp = engine.verify_batch(batch), oracle.verify_batch(batch, threads=2)
    assert_records_equal(got, exp, None, "nothing parses")
    assert all(int(s) != A.ZKE_OK for s in got["status"])
    check_batch(engine, oracle, rag.emails, rag.inter, "ragged again, behind the empty batch")


def test_digest_of_the_empty_message(engine):
    assert bytes(engine.sha256_batch([b""])[0]) == hashlib.sha256(b"").digest()
