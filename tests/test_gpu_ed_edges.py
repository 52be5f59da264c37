"""GPU (-m gpu): edges of the Ed25519 verify entry (engine.ed25519_verify_batch -> ed25519_verify_kernel): every message
length 1..32, S at and around its boundaries (every S + kL that fits 256 bits), and the launch shapes of the
16-signatures-per-wave mapping — n not a multiple of 16, waves in which all quads but one leave early, a wave that leaves as
a whole, and tail quads that replicate signature n-1.  Vectors: ed_vectors.build_edge_vectors(); expectations: ed25519_ref."""
import pytest

import ed_vectors

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def batches():
    return ed_vectors.build_edge_vectors()


def run(engine, batches, prefix):
    picked = [(l, b) for l, b in batches if l.startswith(prefix)]
    assert picked
    for label, batch in picked:
        got = engine.ed25519_verify_batch([v[0] for v in batch], [v[1] for v in batch], [v[2] for v in batch])
        exp = [v[3] for v in batch]
        assert [int(g) for g in got] == exp, "%s: got %s, expected %s; keys %s, signatures %s" % (
            label, list(got), exp, [v[0].hex() for v in batch], [v[2].hex() for v in batch])
    return picked


def test_every_message_length(engine, batches):
    assert len(run(engine, batches, "msg_len")) == 32


def test_s_boundaries(engine, batches):
    picked = run(engine, batches, "S ")
    assert len(picked) == 2 and len(picked[0][1]) >= 14


def test_batch_sizes_around_the_wave(engine, batches):
    assert [len(b) for _, b in run(engine, batches, "n = ")] == [1, 15, 16, 17, 33]


def test_one_valid_quad_among_early_outs(engine, batches):
    picked = run(engine, batches, "one valid signature at quad")
    assert len(picked) == 32
    for _, b in picked:
        assert len(b) == 16 and sorted(v[3] for v in b)[-2:] in ([0, 2], [1, 2])


def test_wave_of_early_outs_then_valid_wave(engine, batches):
    (_, b), = run(engine, batches, "a wave of early-outs")
    assert all(v[3] < 2 for v in b[:16]) and all(v[3] == 2 for v in b[16:]) and len(b) == 32


def test_tail_replicates_the_last_signature(engine, batches):
    (_, b), = run(engine, batches, "17 signatures")
    assert [v[3] for v in b[-2:]] == [1, 2] and len(b) == 17
