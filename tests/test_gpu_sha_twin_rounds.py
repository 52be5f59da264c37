"""GPU (-m gpu): the rounds of sha256_twin_group (csrc/sha256.hip.h) as a lane pair hands them across — inputs that tell a wrong
partner, a B lane whose K + W is not zero, a lost carry and a moved state apart.

The default round keeps Q = h + K + W on A lanes (0 on B lanes), adds the partner's R3 to everybody's W, makes the next round's Q
in place with an add that only A lanes perform and gives the B lanes W[partner] + W.  Message p of a group sits in lanes
8 (p / 4) + p % 4 (A) and 8 (p / 4) + 7 - p % 4 (B).  Engines: the twin forced, and the one that chooses it under four queues,
built as tests/test_gpu_sha_twin.py builds its own.  Everything against hashlib through Engine.sha256_batch, one launch per
check; then one verify batch against the oracle."""
import os

import pytest

import synth
from test_gpu_sha_edges import check_batch, check_digests
from test_gpu_sha_handover import nblk
from test_gpu_sha_twin import engine_with, tag

pytestmark = pytest.mark.gpu

BLOCK_LENS = (55, 119, 183, 247)          # 1, 2, 3 and 4 blocks, each the longest of its count


@pytest.fixture(scope="module")
def engines():
    """(forced twin, chosen under 4 queues)"""
    queues = os.environ.get("GPU_MAX_HW_QUEUES")
    es = [engine_with({"ZKE_SHA_RING": 1, "ZKE_SHA_TWIN": 1, "GPU_MAX_HW_QUEUES": queues}),
          engine_with({"GPU_MAX_HW_QUEUES": 4}, slots=8)]
    yield es
    for e in es:
        e.close()


def test_engines_take_the_twin(engines):
    assert [nblk(x) for x in BLOCK_LENS] == [1, 2, 3, 4]
    for eng in engines:
        assert eng.sha_ring() and eng.sha_twin()


def test_message_p_is_the_byte_p(engines):
    """Two groups in one launch, lengths of 1, 2, 3 and 4 blocks in turn, message p all bytes p: a pair that reads another
    pair's lane, or a B lane that adds a K + W word, yields another message's digest or nobody's."""
    msgs = [bytes([p]) * BLOCK_LENS[p % 4] for p in range(64)]
    for eng in engines:
        check_digests(eng, msgs, f"message p = byte p, {tag(eng)}")


@pytest.mark.parametrize("fill", [0x00, 0xFF])
def test_zero_and_ones_messages_at_the_row_edges(engines, fill):
    """All-0x00 and all-0xFF messages at positions 0, 15, 16 and 31 of both groups (the first and last pair of a DPP row's halves):
    these carry out of h + K + W and out of the in-place add.  The other positions hold the byte-p messages."""
    msgs = [bytes([p]) * BLOCK_LENS[p % 4] for p in range(64)]
    for g in (0, 32):
        for k, pos in enumerate((0, 15, 16, 31)):
            msgs[g + pos] = bytes([fill]) * BLOCK_LENS[(k + g // 32) % 4]
    for eng in engines:
        check_digests(eng, msgs, f"all 0x{fill:02x} at 0, 15, 16, 31, {tag(eng)}")


@pytest.mark.parametrize("pos", [0, 15, 16, 31])
def test_five_blocks_beside_31_of_one(engines, pos):
    """The group runs the rounds of five blocks on 31 messages that finished after the first: their state must not move."""
    msgs = [bytes([p + 1]) * (p % 56) for p in range(32)]
    msgs[pos] = bytes([0xA5]) * 311
    assert nblk(311) == 5 and all(nblk(len(m)) == 1 for i, m in enumerate(msgs) if i != pos)
    for eng in engines:
        check_digests(eng, msgs, f"five blocks at {pos}, {tag(eng)}")


def test_verify_batch_of_33(engines, oracle):
    """33 e-mails through the hash / modexp launch: one full twin group and a group of one per kind."""
    wl = synth.make_workload("twin-rounds-33", 33, 3000, n_keys=4, seed=36, ragged=True)
    for eng in engines:
        check_batch(eng, oracle, wl.emails, wl.inter, f"33 e-mails, {tag(eng)}")
