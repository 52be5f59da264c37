"""GPU (-m gpu): the engine's map of which slots share a hardware queue (zke_engine_queue_count / zke_engine_slot_queue) and the order
in which submission tickets visit the slots (zkemail.rs_amd/csrc/slot_order.hip.h).

On an engine with 10 slots in whatever queue pool the process has, one created with 2 slots and grown to 7, and one with 3: every slot
reports a group wherever slots must share (more slots than queues), the groups are non-empty and numbered by their lowest slot, and
there are at most as many as the pool has queues and as the engine has slots.  Then 3 x slots batches of 8 synthetic e-mails go through
zke_verify_batch_device — each batch its own seed, one e-mail per batch corrupted —: the sequence of slots taken equals the CPU order
applied to the reported map (plain round-robin where the map is unknown: as many queues as slots), and every record is what the signer
expects.  The same batches through zke_verify_batch_async / zke_batch_wait on a 6-slot engine: the tickets name the slots of the same
order and deliver the right records."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import synth
from zkemail_rs_amd import _abi as A

pytestmark = pytest.mark.gpu

N_PER_BATCH = 8


def make_batches(count, seed0=9100):
    """`count` batches of 8 e-mails, batch k from seed seed0 + k, e-mail k % 8 of it corrupted (body and header in turn)."""
    keys = synth.keys_of(2048, 4)
    out = []
    for k in range(count):
        rng = np.random.default_rng(seed0 + k)
        emails, inter = [], []
        for i in range(N_PER_BATCH):
            key = keys[(k + i) % len(keys)]
            body = synth.ascii_body(rng, 200 + 37 * ((k + i) % 5))
            hs = synth.std_headers(rng, 100 * k + i, "example.com")
            corrupt = (("body", "header")[k % 2]) if i == k % N_PER_BATCH else None
            raw, it = synth.sign_email(hs, body, key, synth.SignSpec(domain="example.com"), corrupt=corrupt)
            it["corrupt"] = corrupt
            emails.append(A.Email("example.com", raw, A.PublicKey(key.pkcs1_der, "rsa")))
            inter.append(it)
        out.append((A.PackedBatch(emails), inter))
    return out


def check_records(got, inter, what):
    """status of every e-mail, body and header hash of the valid ones: what the signer expects"""
    assert len(got) == len(inter), what
    for i, it in enumerate(inter):
        if it["corrupt"] is not None:
            assert int(got[i]["status"]) == A.ZKE_DKIM_NOT_PASS, (what, i, int(got[i]["status"]))
            assert int(got[i]["detail"]) == (A.D_BODY_HASH_MISMATCH if it["corrupt"] == "body" else A.D_SIG_MISMATCH), (what, i)
            continue
        assert int(got[i]["status"]) == A.ZKE_OK, (what, i, int(got[i]["status"]), int(got[i]["detail"]))
        assert bytes(got[i]["body_hash"]) == it["body_hash"] and bytes(got[i]["header_hash"]) == it["header_hash"], (what, i)


def queue_pool():
    """The queue pool the engine reckons with: GPU_MAX_HW_QUEUES, or what zke_process_init sets when the host has not."""
    v = os.environ.get("GPU_MAX_HW_QUEUES", "")
    return int(v) if v.isdigit() and int(v) > 0 else 23


def reported_map(eng, slots, what):
    """The engine's map, checked for shape: (n_queues, queue_of).  n_queues 0: unknown, every slot reports -1."""
    nq = eng.queue_count()
    queue_of = [eng.slot_queue(s) for s in range(slots)]
    assert eng.slot_queue(slots) == -1 and eng.slot_queue(64) == -1, what
    assert 0 <= nq <= min(queue_pool(), slots), (what, nq)
    if slots > queue_pool():
        assert nq >= 1, f"{what}: {slots} slots in a pool of {queue_pool()} share queues, and the map is unknown"
    if nq == 0:
        assert queue_of == [-1] * slots, (what, queue_of)
        return nq, queue_of
    assert nq < slots, (what, nq)                       # a queue per slot counts as unknown
    assert all(0 <= q < nq for q in queue_of), (what, queue_of)          # every slot reports a group
    assert sorted(set(queue_of)) == list(range(nq)), (what, queue_of)    # the groups are non-empty
    firsts = [queue_of.index(q) for q in range(nq)]
    assert firsts == sorted(firsts), (what, queue_of)                    # numbered in order of their lowest slot
    return nq, queue_of


def slot_for_ticket(nq, queue_of, t):
    """slot_order.hip.h on the reported map"""
    if nq == 0:
        return t % len(queue_of)
    mine = [s for s, q in enumerate(queue_of) if q == t % nq]
    return mine[(t // nq) % len(mine)]


def run_device_entry():
    """In the child process of test_device_entry_follows_the_reported_map (torch initialises the GPU first)."""
    import torch
    torch.zeros(1, device="cuda")
    import bench
    import zkemail_rs_amd as z
    dev = torch.device("cuda", 0)
    bs = make_batches(30)
    dbs = [bench.device_batch(torch, p, dev) for p, _ in bs]
    max_n, max_raw = N_PER_BATCH, max(int(p.raw_off[-1]) for p, _ in bs)
    for what, created, grown in (("10 slots", 1, 10), ("2 slots grown to 7", 2, 7), ("3 slots", 3, 3)):
        eng = z.Engine(0, slots=created)
        t = 0                                           # tickets count from the engine's creation
        if created > 1:                                 # before the first reserve the map is unknown: plain round-robin
            assert eng.queue_count() == 0 and eng.slot_queue(0) == -1, what
            if created < grown:
                eng.reserve(max_n, max_raw, created, 0)
                nq, queue_of = reported_map(eng, created, what + ", before it grew")
                outs = [torch.zeros(N_PER_BATCH * 192, dtype=torch.uint8, device=dev) for _ in range(3)]
                for k in range(3):
                    cb, keep, totals = dbs[k]
                    eng.verify_batch_device(cb, totals[0], totals[1], totals[2], outs[k].data_ptr(), 0)
                    assert eng.last_slot() == slot_for_ticket(nq, queue_of, t), (what, "before it grew", t)
                    t += 1
                eng.sync()
                for k in range(3):
                    check_records(outs[k].cpu().numpy().view(A.RESULT_DTYPE), bs[k][1], f"{what}, before it grew, batch {k}")
        eng.reserve(max_n, max_raw, grown, 0)
        nq, queue_of = reported_map(eng, grown, what)
        print(f"{what}: {nq} queues, queue_of {queue_of}")
        count = 3 * grown
        outs = [torch.zeros(N_PER_BATCH * 192, dtype=torch.uint8, device=dev) for _ in range(count)]
        taken = []
        for k in range(count):
            cb, keep, totals = dbs[k]
            eng.verify_batch_device(cb, totals[0], totals[1], totals[2], outs[k].data_ptr(), 0)
            taken.append(eng.last_slot())
        want = [slot_for_ticket(nq, queue_of, t + k) for k in range(count)]
        assert taken == want, (what, taken, want)
        if nq == 0:                                     # as many queues as slots: the order is plain round-robin
            assert taken == [(t + k) % grown for k in range(count)], (what, taken)
        else:                                           # every queue takes every nq-th batch
            assert [queue_of[s] for s in taken] == [(t + k) % nq for k in range(count)], (what, taken)
        eng.sync()
        for k in range(count):
            check_records(outs[k].cpu().numpy().view(A.RESULT_DTYPE), bs[k][1], f"{what}, batch {k}")
        eng.close()
    print("slot queues device entry ok")


def test_device_entry_follows_the_reported_map():
    """zke_verify_batch_device on engines of 10, 2 -> 7 and 3 slots.  A subprocess: torch owns the device buffers and has to initialise
    HIP before the engine does."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent(f"""
        import sys
        sys.path.insert(0, {root!r}); sys.path.insert(0, {os.path.join(root, 'tests')!r})
        import test_gpu_slot_queues as T
        T.run_device_entry()
    """)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "slot queues device entry ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_host_tickets_follow_the_reported_map():
    """zke_verify_batch_async / zke_batch_wait on a 6-slot engine: 18 batches back to back, the slot in each ticket's low six bits is the
    order's, and every ticket delivers its own batch's records (waited for out of order)."""
    import zkemail_rs_amd as z
    slots = 6
    bs = make_batches(3 * slots)
    eng = z.Engine(slots=slots, host_threads=2)
    try:
        eng.reserve(N_PER_BATCH, max(int(p.raw_off[-1]) for p, _ in bs), slots, 0)
        eng.reserve_host(N_PER_BATCH, max(int(p.raw_off[-1] + p.domain_off[-1] + p.key_off[-1]) for p, _ in bs))
        nq, queue_of = reported_map(eng, slots, "6 slots")
        pending = []
        for k, (p, _) in enumerate(bs):
            t, out = eng.verify_batch_async(p)
            assert (t & 63) == slot_for_ticket(nq, queue_of, k) == eng.last_slot(), (k, t & 63, nq, queue_of)
            pending.append((t, out))
        for k in list(range(1, len(bs), 2)) + list(range(0, len(bs), 2)):
            eng.wait(pending[k][0])
            check_records(pending[k][1], bs[k][1], f"host ticket of batch {k}")
        for k, (t, out) in enumerate(pending):          # still theirs after every other batch has been delivered
            check_records(out, bs[k][1], f"host batch {k}, at the end")
    finally:
        eng.close()
