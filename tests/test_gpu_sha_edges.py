"""GPU (-m gpu): the three SHA routines — sha256_batch_kernel, sha256_pair_group (csrc/sha256.hip.h) and sha_lane
(csrc/verdict.hip.h) — against hashlib, the Python signer's own hashes and the CPU oracle, on the inputs of
tests/sha_edge_cases.py.  tests/test_sha_order_model.py certifies on the CPU which branches each population reaches
(padding edges, 0x80 / bit-length tile splits, partial chunks, finished rows, the direct and the bucketed job mapping).

Every device run is compared with a CPU reference, never with another device run.  Engines with options of their own
(zke_options.sha_mapping, .slots) run in a child process with its own time limit; a child that ends with a non-zero or
signal status fails the test with its output, and nothing is tried twice.

Default options reach the one-wave kernel in tests 1, 2 and 5 (more than 512 groups of 64 messages); sha_mapping = 1 / 2
puts the same inputs through the other routine."""
import hashlib
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import sha_edge_cases as S
import synth
from zkemail_rs_amd import _abi as A
from test_gpu_verify import assert_records_equal, run_both

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def in_child(body: str, timeout: int = 300):
    """Run `body` (it has z, S, T = this module, orc = the oracle) in a fresh interpreter."""
    code = textwrap.dedent(f"""
        import sys
        sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})
        import oracle_lib, sha_edge_cases as S, test_gpu_sha_edges as T
        import zkemail_rs_amd as z
        orc = oracle_lib.load()
    """) + textwrap.dedent(body) + "\nprint('child ok')\n"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and "child ok" in r.stdout, f"exit {r.returncode}\n" + r.stdout[-3000:] + r.stderr[-3000:]


# ------------------------------------------------------------------ block level
def check_digests(eng, msgs, what):
    got = eng.sha256_batch(msgs)
    bad = [(i, len(m)) for i, m in enumerate(msgs) if bytes(got[i]) != hashlib.sha256(m).digest()]
    assert not bad, f"{what}: {len(bad)} of {len(msgs)} digests differ from hashlib; (index, length) {bad[:12]}"


def test_one_wave_kernel_block_level(engine):
    """1. More than 32 768 messages in one zke_sha256_batch call with default options: sha256_batch_kernel.  Every length of
    EDGE_LENS at every start alignment modulo 16, the wave populations, a last workgroup with a full wave, a wave of 36
    messages and two empty waves."""
    msgs, info = S.block_message_set(S.N_BLOCK)
    assert len(msgs) > 32768
    check_digests(engine, msgs, "one wave per 64 messages, default options")


def test_block_level_through_both_forced_mappings():
    """1, continued: the same messages through sha_mapping = 2 (the pair routine above its threshold) and, cut to fewer
    than 32 768 messages, through sha_mapping = 1 (the one-wave kernel below it)."""
    in_child("""
        msgs, info = S.block_message_set(S.N_BLOCK)
        eng = z.Engine(sha_mapping=2)
        T.check_digests(eng, msgs, "sha_mapping = 2")
        eng.close()
        eng = z.Engine(sha_mapping=1)
        assert info["n_edge"] <= S.N_BLOCK_CUT < 32768
        T.check_digests(eng, msgs[:S.N_BLOCK_CUT], "sha_mapping = 1")
        T.check_digests(eng, [b"abc"], "sha_mapping = 1, one message")
        eng.close()
    """)


def test_threshold_between_the_two_kernels(engine):
    """2. The same messages at n = 32 768 (512 groups: the pair routine) and n = 32 769 (513: the one-wave kernel)."""
    msgs, _ = S.block_message_set(32769, max_len=70000)
    check_digests(engine, msgs[:32768], "n = 32768")
    check_digests(engine, msgs, "n = 32769")


# ------------------------------------------------------------------ pipeline
def check_batch(eng, orc, emails, inter, what):
    """records = the oracle's; both hashes = the signer's; every e-mail that was not corrupted on purpose is ZKE_OK"""
    batch = A.PackedBatch(emails)
    got = eng.verify_batch(batch)
    exp = orc.verify_batch(batch, threads=16)
    assert_records_equal(got, exp, None, what)
    n_ok = 0
    for i, it in enumerate(inter):
        if it is None or it.get("corrupt") is not None:
            assert int(got[i]["status"]) != A.ZKE_OK, (what, i)
            continue
        assert int(got[i]["status"]) == A.ZKE_OK, (what, i, int(got[i]["status"]), int(got[i]["detail"]))
        assert bytes(got[i]["body_hash"]) == it["body_hash"] and bytes(got[i]["header_hash"]) == it["header_hash"], (what, i)
        assert int(got[i]["canon_body_len"]) == it["hashed_body_len"] and int(got[i]["canon_header_len"]) == len(it["canon_header"]), (what, i)
        n_ok += 1
    assert n_ok == sum(1 for it in inter if it is not None and it.get("corrupt") is None)
    return got


def run_padding_edges(z, orc):
    big = S.pipeline_population()
    hdr = S.header_sweep()
    S.interleave_check(big[1]); S.interleave_check(hdr[1])
    for opts, name in ((dict(), "default"), (dict(sha_mapping=1), "sha_mapping = 1")):
        eng = z.Engine(**opts)
        check_batch(eng, orc, big[0], big[1], f"padding edges, {name}")
        check_batch(eng, orc, hdr[0], hdr[1], f"header sweep, {name}")
        eng.close()


def test_padding_edges_through_the_pipeline_both_algorithms():
    """3. Body lengths over EDGE_LENS (1 MiB included), 256 consecutive header-preimage lengths, from_domain of 55 / 56 / 63 /
    64 bytes; rsa-sha256 and rsa-sha1 neighbours in the batch; c=relaxed and c=simple.  Once as one batch (bucketed mapping)
    and the header sweep alone (direct mapping), each on a default engine (the pair routine and, for groups with a SHA-1
    job, its one-wave fallback) and on a sha_mapping = 1 engine (sha256_batch_kernel, then the RSA roles in a launch of
    their own)."""
    in_child("T.run_padding_edges(z, orc)", timeout=420)


def run_length_buckets(z, orc):
    eng = z.Engine(slots=1)
    uni = S.uniform_batch()
    for name, (emails, inter) in S.bucket_populations().items():
        for rep in range(2):
            check_batch(eng, orc, emails, inter, f"{name}, run {rep}")
        check_batch(eng, orc, uni[0], uni[1], f"uniform batch behind {name}")          # stale counters would misplace its jobs
    eng.close()


def test_length_buckets_certified_populations():
    """4. The populations test_sha_order_model.py::test_census_bucket_populations certifies — direct with hi - lo == 1 across
    two lanes' counters, bucketed with hi - lo == 2, groups over three classes, cut groups, skipped groups, classes >= 16,
    n not a multiple of 256, e-mails without a message — in one slot, each twice, each followed by a uniform batch."""
    in_child("T.run_length_buckets(z, orc)", timeout=300)


def test_split_launch_at_its_real_size(engine, oracle):
    """5. 8 200 e-mails with default options: n_pad = 8 256, 516 groups — sha256_batch_kernel over the whole job list in
    arrival order, then the RSA roles alone; the front end still files the length buckets, nothing consumes them and the
    verdict launch clears them.  Then a ragged 700-e-mail batch in the same slot (bucketed, fused), then the large batch again."""
    kw = dict(rsa_bits=2048, n_keys=8, ragged=True, chunk=520)
    a = synth.make_workload_parallel("split256", 6150, 600, seed=81, invalid_frac=0.05, **kw)
    b = synth.make_workload_parallel("split1", 2050, 600, seed=82, invalid_frac=0.05, algo="rsa-sha1", **kw)
    emails, inter = [], []
    for k in range(2050):                                        # three rsa-sha256 e-mails, one rsa-sha1
        emails += a.emails[3 * k:3 * k + 3] + [b.emails[k]]
        inter += a.inter[3 * k:3 * k + 3] + [b.inter[k]]
    assert len(emails) == 8200 and 4 * ((8200 + 63) // 64) == 516
    n_bad = sum(it["corrupt"] is not None for it in inter)
    assert 100 < n_bad < 1000
    small = synth.make_workload_parallel("ragged700", 700, 20000, seed=83, invalid_frac=0.1, chunk=350, **{k: v for k, v in kw.items() if k != "chunk"})
    exp_big = oracle.verify_batch(A.PackedBatch(emails), threads=16)
    exp_small = oracle.verify_batch(A.PackedBatch(small.emails), threads=16)
    pb, ps = A.PackedBatch(emails), A.PackedBatch(small.emails)
    for step, (p, exp) in enumerate(((pb, exp_big), (ps, exp_small), (pb, exp_big))):
        got = engine.verify_batch(p)
        for f in (f for f in A.RESULT_DTYPE.names if f != "reserved"):
            g, x = np.asarray(got[f]), np.asarray(exp[f])
            bad = np.nonzero((g != x).reshape(len(g), -1).any(axis=1))[0]
            assert len(bad) == 0, f"step {step}: field {f} differs from the oracle at records {bad[:8]}"
    got = engine.verify_batch(pb)
    for i, it in enumerate(inter):
        if it["corrupt"] is None:
            assert int(got[i]["status"]) == A.ZKE_OK and bytes(got[i]["body_hash"]) == it["body_hash"] and bytes(got[i]["header_hash"]) == it["header_hash"], i
    assert int((np.asarray(got["status"]) == 0).sum()) == 8200 - n_bad


# ------------------------------------------------------------------ later signature rounds
def run_signature_rounds(z, orc):
    import torch
    torch.zeros(1, device="cuda")
    import bench
    cs, nbad = S.signature_round_emails()
    emails = [c.email for c in cs]
    eng = z.Engine(0)
    got, exp, d1, d2 = run_both(eng, orc, emails)                                  # the host entry
    dev = torch.device("cuda", 0)
    packed = A.PackedBatch(emails)
    cb, keep, totals = bench.device_batch(torch, packed, dev)
    out = torch.zeros(packed.n * 192, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    eng.verify_batch_device(cb, totals[0], totals[1], totals[2], out.data_ptr(), 0)   # the device entry
    eng.sync()
    got_dev = out.cpu().numpy().view(A.RESULT_DTYPE)
    for what, g in (("host entry", got), ("device entry", got_dev)):
        assert_records_equal(g, exp, None, f"signature rounds, {what}")
        assert [int(x) for x in g["sig_index"]] == nbad, what
        for i, c in enumerate(cs):
            assert int(g[i]["status"]) == A.ZKE_OK, (what, i, int(g[i]["status"]), int(g[i]["detail"]))
            assert bytes(g[i]["body_hash"]) == c.inter["body_hash"] and bytes(g[i]["header_hash"]) == c.inter["header_hash"], (what, i)
            assert int(g[i]["canon_body_len"]) == c.inter["hashed_body_len"], (what, i)
    for i, c in enumerate(cs):
        k = len(c.inter["em"])
        assert bytes(d1.em[i, :k]) == c.inter["em"] == bytes(d2.em[i, :k]), i
    eng.close()


def test_one_lane_routine_in_later_signature_rounds():
    """6. sha_lane: one and three failing same-domain signatures in front of the good one, whose hashed body runs over every
    edge length up to 4 097 (l= shorter than the body) and whose header preimage runs over 130 consecutive lengths; rsa-sha256
    and rsa-sha1, c=relaxed and c=simple; through the host entry and the device entry."""
    in_child("T.run_signature_rounds(z, orc)", timeout=420)


def test_sha_mapping_out_of_range_is_refused():
    import zkemail_rs_amd as z
    with pytest.raises(z.EngineError):
        z.Engine(sha_mapping=3)
