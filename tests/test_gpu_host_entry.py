"""-m gpu: the host-memory entry point as a drop-in caller uses it (core/src/circuits.rs:9 takes a RAM-resident &Email) — the
asynchronous form through several submission slots, re-entrancy from many host threads on ONE engine (SURVEY §8(b) Threading:
the reference's functions are re-entrant), slot timings, and the error path's slot hygiene."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

from zkemail_rs_amd import _abi as A

import body_cases
import body_model
import cases
import synth
import test_gpu_qp_map as QM
from test_gpu_verify import assert_records_equal

pytestmark = pytest.mark.gpu


def _batches(count, n=96, seed0=300):
    """`count` different batches (ragged bodies, a few invalid e-mails) and the oracle-independent expectation per e-mail."""
    out = []
    for k in range(count):
        wl = synth.make_workload("host", n + 7 * k, 3000, rsa_bits=2048, n_keys=4, seed=seed0 + k, ragged=True, invalid_frac=0.1)
        out.append((A.PackedBatch(wl.emails), wl))
    return out


def test_async_host_entry_through_slots(oracle):
    """zke_verify_batch_async: 5 slots, 23 batches of 6 different shapes submitted back to back (each waits only when its slot
    comes round again — a slot whose batch was never waited for delivers it before it is reused), out of order waits, double
    waits; every record equal to the oracle's and to the synchronous entry's."""
    import zkemail_rs_amd as z
    eng = z.Engine(slots=5, host_threads=4)
    try:
        bs = _batches(6)
        exp = [oracle.verify_batch(p, threads=4) for p, _ in bs]
        eng.reserve(max(p.n for p, _ in bs), max(int(p.raw_off[-1]) for p, _ in bs), 5, 0)
        eng.reserve_host(max(p.n for p, _ in bs), max(int(p.raw_off[-1] + p.domain_off[-1] + p.key_off[-1]) for p, _ in bs))
        pending = []
        for i in range(23):
            p, wl = bs[i % len(bs)]
            t, out = eng.verify_batch_async(p)
            pending.append((t, out, i % len(bs)))
        # the first 18 were retired by their slots' later batches: their records are there without a wait
        for t, out, k in pending[:18]:
            assert_records_equal(out, exp[k], None, f"retired by reuse (batch shape {k})")
        for t, out, k in reversed(pending):         # waits in reverse order, then once more
            eng.wait(t)
            assert_records_equal(out, exp[k], None, f"async batch shape {k}")
        for t, out, k in pending:
            eng.wait(t)
        # the synchronous wrapper and the single-e-mail entry share the path
        for (p, wl), e in zip(bs[:2], exp):
            assert_records_equal(eng.verify_batch(p), e, None, "sync wrapper")
        n_ok = sum(int((e["status"] == 0).sum()) for e in exp)
        assert n_ok == sum(sum(1 for it in wl.inter if it["corrupt"] is None) for _, wl in bs)
        # an empty batch is a no-op with a ticket that is already done
        t, out = eng.verify_batch_async(A.PackedBatch([]))
        eng.wait(t)
        with pytest.raises(z.EngineError):
            eng.wait((10 ** 9 << 6) | 1)
    finally:
        eng.close()


def test_four_threads_one_engine_records_identical_to_serial():
    """4 host threads x 50 batches on one engine with 3 slots (so threads share slots), host and device entry and regex batches
    mixed: every record identical to a serial run.  (A subprocess: torch must initialise the GPU before the engine does in a process that
    uses both.)"""
    import os, subprocess, sys, textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent(f"""
        import sys, threading
        sys.path.insert(0, {root!r}); sys.path.insert(0, {os.path.join(root, 'tests')!r})
        import numpy as np, torch
        torch.zeros(1, device="cuda")
        import bench, oracle_lib, synth, zkemail_rs_amd as z
        from zkemail_rs_amd import _abi as A
        from test_gpu_host_entry import _batches
        from test_gpu_verify import assert_records_equal
        oracle = oracle_lib.load()
        eng = z.Engine(slots=3, host_threads=2)
        bs = _batches(4, n=64, seed0=400)
        serial = [eng.verify_batch(p).copy() for p, _ in bs]
        for (p, _), s in zip(bs, serial):
            assert_records_equal(s, oracle.verify_batch(p, threads=4), None, "serial run")
        # regex batches too (the registry's read path and the slots' regex workspaces under the same traffic)
        rx = []
        for k in range(3):
            inputs, _, _ = synth.make_regex_workload("thr", 40 + 9 * k, 2000, n_header_parts=1 + k % 2, n_body_parts=k % 2, qp_frac=0.05, fail_frac=0.2, seed=450 + k)
            rx.append(eng.pack_with_regex(inputs))
            assert_records_equal(eng.verify_batch(rx[-1]), oracle.verify_batch(oracle.pack_with_regex(inputs), threads=4), None, "serial regex run")
        rx_serial = [eng.verify_batch(p).copy() for p in rx]
        dev = torch.device("cuda", 0)
        dbs = [bench.device_batch(torch, p, dev) for p, _ in bs]
        errors = []

        def worker(tid):
            try:
                outs_dev = [torch.zeros(p.n * 192, dtype=torch.uint8, device=dev) for p, _ in bs]
                for it in range(50):
                    k = (tid + it) % len(bs)
                    p = bs[k][0]
                    if it % 5 == 4:                     # a regex batch through the host entry
                        r = (tid + it) % len(rx)
                        got = eng.verify_batch(rx[r])
                        for f in A.RESULT_DTYPE.names:
                            if f != "reserved" and not (np.asarray(got[f]) == np.asarray(rx_serial[r][f])).all():
                                raise AssertionError(f"thread {{tid}} iteration {{it}}: regex batch, field {{f}} differs from the serial run")
                        continue
                    if it % 3 == 2:                     # the device-resident entry from the same thread
                        cb, keep, totals = dbs[k]
                        outs_dev[k].zero_()
                        torch.cuda.synchronize()
                        eng.verify_batch_device(cb, totals[0], totals[1], totals[2], outs_dev[k].data_ptr(), 0)
                        eng.sync()
                        got = outs_dev[k].cpu().numpy().view(A.RESULT_DTYPE)
                    elif it % 3 == 1:
                        t, got = eng.verify_batch_async(p)
                        eng.wait(t)
                    else:
                        got = eng.verify_batch(p)
                    for f in A.RESULT_DTYPE.names:
                        if f != "reserved" and not (np.asarray(got[f]) == np.asarray(serial[k][f])).all():
                            raise AssertionError(f"thread {{tid}} iteration {{it}}: field {{f}} differs from the serial run")
            except Exception as ex:
                errors.append(repr(ex))

        ths = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
        for t in ths:
            t.start()
        for t in ths:
            t.join(timeout=300)
        assert not errors, errors[:3]
        assert not any(t.is_alive() for t in ths)
        eng.close()
        print("threads ok")
    """)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "threads ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_slot_timings_and_names(oracle):
    """zke_timings names the three launches; a slot that has not run a timed batch reports zeros (not another slot's figures)."""
    import zkemail_rs_amd as z
    eng = z.Engine(slots=3)
    try:
        (p, wl), = _batches(1, n=128, seed0=500)
        eng.set_timing(True)
        eng.verify_batch(p)                                  # slot 0
        t0 = eng.slot_timings(0)
        assert t0["front_end_us"] > 0 and t0["hash_modexp_us"] > 0 and t0["ed_verdict_us"] > 0 and t0["h2d_us"] > 0 and t0["d2h_us"] > 0
        assert t0["regex_prep_us"] == 0 and t0["dfa_us"] == 0
        assert abs(t0["total_us"] - (t0["front_end_us"] + t0["hash_modexp_us"] + t0["ed_verdict_us"])) < 1.0
        t2 = eng.slot_timings(2)
        assert all(v == 0 for v in t2.values()), t2
        assert eng.timings() == t0                            # the slot used most recently
        with pytest.raises(z.EngineError):
            eng.slot_timings(7)
    finally:
        eng.close()


def test_single_email_entry_and_larger_than_reserved(oracle):
    """zke_verify_email through the pinned path (a batch of one), then a batch larger than anything reserved (the staging and
    the workspace grow), then small again."""
    import zkemail_rs_amd as z
    eng = z.Engine()
    try:
        c = [x for x in cases.build_cases() if x.status == A.ZKE_OK][:5]
        for x in c:
            out = eng.verify_email(x.email)
            w = cases.expected_witness(x)
            assert (out.from_domain_hash, out.public_key_hash) == w
        (small, _), (big, _) = _batches(1, n=8, seed0=600)[0], _batches(1, n=700, seed0=601)[0]
        for p in (small, big, small):
            assert_records_equal(eng.verify_batch(p), oracle.verify_batch(p, threads=4), None, f"n={p.n}")
    finally:
        eng.close()


def test_length_buckets_across_slot_reuse(oracle):
    """The hash stage files bodies and header preimages under length classes (csrc/sha256.hip.h, ShaOrder) and every slot
    carries its counters from batch to batch (the verdict launch clears them).  One slot, batches that alternate between ragged
    (3 B .. 40 KB bodies, invalid e-mails, rsa-sha1), uniform and tiny: every record equal to the oracle's every time."""
    import zkemail_rs_amd as z
    eng = z.Engine(slots=1)
    try:
        shapes = [dict(n=700, body_len=40000, ragged=True, invalid_frac=0.1), dict(n=300, body_len=4096),
                  dict(n=515, body_len=20000, ragged=True, algo="rsa-sha1"), dict(n=3, body_len=100),
                  dict(n=1100, body_len=9000, ragged=True, invalid_frac=0.3), dict(n=64, body_len=3)]
        packs = []
        for k, sh in enumerate(shapes):
            wl = synth.make_workload_parallel("buckets", rsa_bits=2048, n_keys=8, seed=700 + k, chunk=256, **sh)
            p = A.PackedBatch(wl.emails)
            packs.append((p, oracle.verify_batch(p, threads=8), wl))
        for rep in range(2):
            for k, (p, exp, wl) in enumerate(packs):
                assert_records_equal(eng.verify_batch(p), exp, None, f"pass {rep} shape {k}")
        # the same through the asynchronous entry, all in flight behind each other in the one slot
        pending = [(eng.verify_batch_async(p), exp) for p, exp, _ in packs]
        for (t, out), exp in pending:
            eng.wait(t)
            assert_records_equal(out, exp, None, "async")
        n_ok = int((packs[0][1]["status"] == 0).sum())
        assert n_ok == sum(1 for it in packs[0][2].inter if it["corrupt"] is None) and 0 < n_ok < 700
    finally:
        eng.close()


def test_host_offsets_are_checked(oracle):
    """Offset arrays in host memory are validated before anything is staged (csrc/host_entry.hip.h, host_batch): a length
    that comes out negative is ZKE_E_ARG, not a copy outside the blob; the engine stays usable."""
    import zkemail_rs_amd as z
    eng = z.Engine()
    try:
        (p, _) = _batches(1, n=16, seed0=650)[0]
        good = eng.verify_batch(p)
        for arr in (p.raw_off, p.domain_off, p.key_off):
            keep = arr.copy()
            arr[5], arr[6] = keep[6], keep[5]                      # (the arrays are the ones the zke_batch points to)
            if arr[5] == arr[6]:
                arr[5] += 1
            with pytest.raises(z.EngineError, match="non-decreasing"):
                eng.verify_batch(p)
            with pytest.raises(z.EngineError, match="non-decreasing"):
                eng.verify_batch_async(p)
            arr[:] = keep
        assert_records_equal(eng.verify_batch(p), good, None, "after the refused batches")
    finally:
        eng.close()


def test_scattered_emails_entry_equals_the_packed_one(oracle):
    """zke_verify_emails / _async: the e-mails handed over one by one, each in buffers of its own (what `&[Email]` is in the
    reference), gathered by the engine into its staging image — records identical to zke_verify_batch over the concatenated
    blobs, for ragged batches with invalid and empty e-mails, n = 0 / 1 / 700, through slot reuse and from two threads."""
    import zkemail_rs_amd as z
    eng = z.Engine(slots=3, host_threads=3)
    try:
        assert len(eng.verify_emails([])) == 0
        shapes = _batches(3, n=90, seed0=700) + _batches(1, n=700, seed0=710) + _batches(1, n=1, seed0=720)
        lists = []
        for p, wl in shapes:
            ems = list(wl.emails)
            if len(ems) > 5:      # an empty e-mail, an empty domain and an empty key in the middle of the gather
                ems[3] = A.Email("example.com", b"", ems[3].public_key)
                ems[4] = A.Email("", ems[4].raw_email, ems[4].public_key)
                ems[5] = A.Email("example.com", ems[5].raw_email, A.PublicKey(b"", "rsa"))
            lists.append(ems)
        want = [eng.verify_batch(A.PackedBatch(ems)) for ems in lists]
        for ems, w in zip(lists, want):
            assert_records_equal(w, oracle.verify_batch(A.PackedBatch(ems), threads=4), None, "packed entry")
            assert_records_equal(eng.verify_emails(ems), w, None, f"scattered entry, n={len(ems)}")
        # asynchronous, more batches than slots, waited for out of order
        refs = [A.EmailRefs(ems) for ems in lists]
        pend = [eng.verify_emails_async(refs[k % len(refs)]) for k in range(8)]
        for k in (7, 0, 3, 1, 2, 6, 5, 4):
            eng.wait(pend[k][0])
            assert_records_equal(pend[k][1], want[k % len(refs)], None, f"async scattered batch {k}")
        errors = []

        def worker(tid):
            try:
                for it in range(30):
                    k = (tid + it) % len(lists)
                    got = eng.verify_emails(refs[k]) if it % 2 else eng.verify_batch(A.PackedBatch(lists[k]))
                    assert_records_equal(got, want[k], None, f"thread {tid} iteration {it}")
            except Exception as ex:
                errors.append(repr(ex))
        ths = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
        for t in ths:
            t.start()
        for t in ths:
            t.join(timeout=300)
        assert not errors, errors[:2]
        # a null buffer with a length is refused, and the engine stays usable
        bad = A.EmailRefs(lists[0][:4])
        bad.arr[2].raw = None
        with pytest.raises(z.EngineError, match="null buffer"):
            eng.verify_emails(bad)
        assert_records_equal(eng.verify_emails(refs[0]), want[0], None, "after the refused call")
    finally:
        eng.close()


def test_scattered_regex_entry_equals_the_packed_one(oracle):
    """zke_verify_emails_with_regex: `&[EmailWithRegex]` with the e-mails in their own buffers and the capture tables as
    zke_batch has them — header and body parts, captures that pass and fail, a batch without any capture string."""
    import zkemail_rs_amd as z
    eng = z.Engine(slots=2)
    try:
        for cfg in (dict(n=80, body_len=2500, n_header_parts=2, n_body_parts=1, qp_frac=0.05, fail_frac=0.25, seed=31),
                    dict(n=33, body_len=900, n_header_parts=1, n_body_parts=0, fail_frac=0.3, seed=32)):
            inputs, wl, _ = synth.make_regex_workload("scat", **cfg)
            want = eng.verify_batch(eng.pack_with_regex(inputs))
            assert_records_equal(want, oracle.verify_batch(oracle.pack_with_regex(inputs), threads=4), None, "packed regex entry")
            assert_records_equal(eng.verify_emails_with_regex(inputs), want, None, f"scattered regex entry {cfg}")
            if cfg["n_body_parts"]:
                assert (np.asarray(want["status"]) == 0).sum() > 5 and (np.asarray(want["status"]) != 0).sum() > 5
        bare = [A.EmailWithRegex(i.email, A.RegexInfo([A.CompiledRegex(p.verify_re, None) for p in i.regex_info.header_parts], None)) for i in inputs]
        assert_records_equal(eng.verify_emails_with_regex(bare), eng.verify_batch(eng.pack_with_regex(bare)), None, "no capture strings at all")
    finally:
        eng.close()


def test_engine_lifecycle_returns_its_memory(oracle):
    """40 engines created, used (host entry, gathering entry, a regex batch, the device-mode reserve) and destroyed one after
    the other: device memory free after the last is what it was after the first (no workspace, staging image, DFA table or key
    cache left behind), and every one of them answers like the first."""
    import ctypes as C
    import zkemail_rs_amd as z
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(), C.c_size_t()

    def free_now():
        assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        return free.value
    (p, wl) = _batches(1, n=200, seed0=800)[0]
    inputs, _, _ = synth.make_regex_workload("life", 40, 1500, n_header_parts=1, n_body_parts=1, qp_frac=0.05, seed=801)
    want = want_rx = None
    after_first = None
    for k in range(40):
        eng = z.Engine(slots=4, host_threads=2)
        try:
            eng.reserve(256, 1 << 20, 4, 2)
            got = eng.verify_batch(p)
            got2 = eng.verify_emails(list(wl.emails))
            rx = eng.verify_batch(eng.pack_with_regex(inputs))
            if want is None:
                want, want_rx = got.copy(), rx.copy()
                assert_records_equal(want, oracle.verify_batch(p, threads=4), None, "first engine")
            assert_records_equal(got, want, None, f"engine {k}")
            assert_records_equal(got2, want, None, f"engine {k}, gathering entry")
            assert_records_equal(rx, want_rx, None, f"engine {k}, regex")
        finally:
            eng.close()
        if after_first is None:
            after_first = free_now()
    assert abs(free_now() - after_first) <= (64 << 20), (free_now(), after_first)       # (the runtime keeps a few MB of its own)
    # an engine destroyed with batches nobody waited for delivers them on the way out (include/zkemail_amd.h: `out` stays valid
    # until zke_batch_wait — or zke_engine_destroy — has returned)
    eng = z.Engine(slots=3)
    pend = [eng.verify_batch_async(p) for _ in range(3)]
    eng.close()
    for _, rec in pend:
        assert_records_equal(rec, want, None, "delivered by zke_engine_destroy")


def test_unwaited_batches_with_short_buffers_are_retired_by_the_next_batch():
    """One slot; a scan, a key-record decode, an extraction and a body extraction are submitted asynchronously, each with its
    variable-size buffer too small (sel_blob, keys, cap_blob, bytes of capacity 0), and never waited for.  The slot's next batch
    retires each: that batch is not disturbed (it returns 0, its record is right), the unwaited batch's fixed-size outputs are there
    with the exact *_need, and the shortfall — which had nobody to be told to — does not come back from a later wait on the old
    ticket.  A mapped extraction's origins arrive the same way, with the batch that retires it."""
    import base64
    import re
    import zkemail_rs_amd as z
    from zkemail_rs_amd.engine import _KeyrecBuffers, _ScanBuffers
    c = [x for x in cases.build_cases() if x.status == A.ZKE_OK][0]
    key = c.email.public_key.key
    subject = re.findall(rb"subject:([^\r\n]+)\r\n", c.inter["canon_header"])
    assert len(subject) == 1
    eng = z.Engine(slots=1)
    try:
        def next_batch_retires(ticket):
            got = eng.verify_emails([c.email])
            assert int(got[0]["status"]) == c.status == A.ZKE_OK
            assert (bytes(got[0]["from_domain_hash"]), bytes(got[0]["public_key_hash"])) == cases.expected_witness(c)
            assert bytes(got[0]["body_hash"]) == c.inter["body_hash"] and bytes(got[0]["header_hash"]) == c.inter["header_hash"]
            assert eng.lib.zke_batch_wait(eng.h, ticket) == 0

        # a scan whose selector blob holds nothing
        t, sb = eng.scan_signatures_async([c.email.raw_email], [c.email.from_domain], 8, blob_bytes=0)
        next_batch_retires(t)
        assert [int(x) for x in sb.status[0]] == [A.ZKE_OK, 0, 1, 1] and [int(x) for x in sb.sig_off] == [0, 1]
        assert (int(sb.c.sigs_need), int(sb.c.n_sigs), int(sb.c.sel_blob_need)) == (1, 1, len("sel1"))
        assert (int(sb.sigs[0]["code"]), int(sb.sigs[0]["sel_len"])) == (0, len("sel1"))
        # a decode of the e-mail's key record whose key buffer holds nothing
        kb = _KeyrecBuffers([b"v=DKIM1; k=rsa; p=" + base64.b64encode(key)], 0)
        tk = C.c_uint64()
        assert eng.lib.zke_decode_key_records_async(eng.h, kb.arr, kb.m, A.KEYREC_DNS, C.byref(kb.c), C.byref(tk)) == 0
        next_batch_retires(tk.value)
        assert (int(kb.c.infos_need), int(kb.c.keys_need)) == (1, len(key))
        assert [int(kb.infos[0][f]) for f in ("code", "key_type", "key_off", "key_len")] == [0, A.KEY_RSA, 0, len(key)]
        # an extraction of one header pattern's one group whose string blob holds nothing
        _, dfa_id, prog_id = eng.compile_pattern(synth.HEADER_PATTERNS[1][0], False)
        group = np.array([1], np.uint32)
        part = (A.zke_capture_part * 1)()
        part[0].dfa_id, part[0].prog_id, part[0].n_groups, part[0].groups = dfa_id, prog_id, 1, group.ctypes.data
        refs = A.EmailRefs([c.email])
        out = np.zeros(1, dtype=A.RESULT_DTYPE)
        spans, flags, cap_off, cap_str_off = np.zeros(2, np.uint32), np.full(1, 9, np.uint8), np.full(2, 9, np.uint32), np.full(2, 9, np.uint32)
        o = A.zke_capture_out()
        o.spans, o.spans_cap, o.flags, o.flags_cap = spans.ctypes.data, 2, flags.ctypes.data, 1
        o.cap_off, o.cap_off_cap, o.cap_str_off, o.cap_str_off_cap = cap_off.ctypes.data, 2, cap_str_off.ctypes.data, 2
        o.cap_blob, o.cap_blob_cap = None, 0
        tc = C.c_uint64()
        assert eng.lib.zke_extract_captures_async(eng.h, refs.arr, 1, part, 1, part, 0, out.ctypes.data, C.byref(o), C.byref(tc)) == 0
        next_batch_retires(tc.value)
        assert int(out[0]["status"]) == A.ZKE_OK and bytes(out[0]["header_hash"]) == c.inter["header_hash"]
        assert (int(o.n_strings), int(o.cap_blob_need)) == (1, len(subject[0]))
        assert [int(x) for x in cap_off] == [0, 1] and [int(x) for x in cap_str_off] == [0, len(subject[0])] and int(flags[0]) == 0
        assert int(spans[1]) - int(spans[0]) == len(subject[0])
        # a body extraction whose byte buffer holds nothing: the info and the exact need, by the model
        kind, want = body_model.verdict(c.email.raw_email, False)
        assert kind == "ok" and len(want.data) > 0
        tb, bb = eng.extract_bodies_async([c.email.raw_email], body_bytes=0)
        next_batch_retires(tb)
        assert (int(bb.c.infos_need), int(bb.c.bytes_need)) == (1, len(want.data))
        assert [int(bb.infos[0][f]) for f in ("status", "detail", "part", "encoding", "src_off", "src_len", "body_len", "reserved", "body_off")] == \
            [A.ZKE_OK, 0, want.part, want.encoding, want.src_off, want.src_len, len(want.data), 0, 0]
        # a mapped extraction (a header part and a body part: the origin launch runs) nobody waits for: spans, strings AND origins are
        # there once the next batch has retired it, and they are what the synchronous entry delivers
        parts = QM.parts_of(eng, [synth.HEADER_PATTERNS[1], _body_word_pattern(c)])
        st = QM.run_extract(eng, [c.email], parts, 1, mapped=True, asynchronous=True)
        next_batch_retires(st["ticket"].value)
        ref = QM.run_extract(eng, [c.email], parts, 1, mapped=True)
        assert int(ref["out"][0]["status"]) == A.ZKE_OK and (ref["spans"] != QM.NO).all()
        assert QM.delivered(st) == QM.delivered(ref)
        assert st["ospans"].tolist() == ref["ospans"].tolist() and st["oflags"].tolist() == ref["oflags"].tolist() == [0, 0]
    finally:
        eng.close()


def _body_word_pattern(c):
    """A body pattern that matches exactly once in a case's e-mail: the first word of the body's last line, the word behind it as group 1."""
    import re
    body = c.email.raw_email.split(b"\r\n\r\n", 1)[1]
    m = re.search(rb"\r\n([A-Za-z0-9]{4,}) ([A-Za-z0-9]+)[^\r\n]*\r\n$", body)
    assert m and body.count(m.group(1)) == 1, body[-200:]
    return (m.group(1).decode() + " ([A-Za-z0-9]+)", [1])


def test_every_side_output_in_turn_on_one_slot():
    """Every kind of pending delivery through ONE slot, one after the other, none waited for: a scan, a lone key-record decode, a body
    extraction, a selection from records, a mapped extraction, a plain verify — each retired by the submission behind it, the last by
    its wait.  Every output equals what the synchronous entry returns for the same call on a fresh engine, and waiting on the old
    tickets afterwards returns 0.  Then the same sequence through two slots, waited for in reverse order.  Three signed e-mails of
    the case list; behind them two unsigned ones for the body extraction: the golden qp_lone_lf_lines.eml, and the case whose body
    outgrows its e-mail, so that a second place is in use."""
    import base64
    import zkemail_rs_amd as z
    good = [x for x in cases.build_cases() if x.status == A.ZKE_OK and x.email.public_key.key_type == "rsa"][:3]
    assert len(good) == 3
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "body_cases", "qp_lone_lf_lines.eml"), "rb") as f:
        lone_lf = f.read()
    outgrows = dict(body_cases.all_cases())["qp_lf_lines_outgrow_the_email"]
    emails = [x.email for x in good] + [A.Email("example.com", raw, good[0].email.public_key) for raw in (lone_lf, outgrows)]
    raws, doms = [e.raw_email for e in emails], [e.from_domain for e in emails]
    record = lambda e: b"v=DKIM1; k=rsa; p=" + base64.b64encode(e.public_key.key)
    records = [record(e) for e in emails[:3]] + [b"v=DKIM1; p=", None]
    cand = [[b"v=DKIM1; k=rsa; p=AAAA", record(emails[0])], [record(emails[1])], [], [record(emails[0])], [None, record(emails[2])]]
    patterns = [synth.HEADER_PATTERNS[1], _body_word_pattern(good[0])]

    def submit_all(eng, parts):
        """The six submissions in turn; returns (tickets, a function that reads every output once they have been delivered)."""
        t1, scan = eng.scan_signatures_async(raws, doms, 8)
        t2, keyrec = eng.decode_key_records_async(records)
        t3, bodies = eng.extract_bodies_async(raws)
        t4, sel_out, sel_chosen, sel_keys = eng.select_keys_from_records_async(emails, cand)
        ext = QM.run_extract(eng, emails, parts, 1, mapped=True, asynchronous=True)
        refs = A.EmailRefs(emails)
        t6, recs = eng.verify_emails_async(refs)

        def outputs():
            return dict(scan=scan.result(), keyrec=keyrec.result(), bodies=bodies.result(), sel_out=sel_out, sel_chosen=sel_chosen.tolist(),
                        sel_keys=sel_keys.result(), ext=QM.delivered(ext), ospans=ext["ospans"].tolist(), oflags=ext["oflags"].tolist(), recs=recs, keep=refs)
        return [t1, t2, t3, t4, ext["ticket"].value, t6], outputs

    fresh = z.Engine()
    try:
        parts = QM.parts_of(fresh, patterns)
        sel = fresh.select_keys_from_records(emails, cand)
        ext = QM.run_extract(fresh, emails, parts, 1, mapped=True)
        want = dict(scan=fresh.scan_signatures(raws, doms, 8), keyrec=fresh.decode_key_records(records), bodies=fresh.extract_bodies(raws),
                    sel_out=sel[0], sel_chosen=sel[1].tolist(), sel_keys=sel[2], ext=QM.delivered(ext), ospans=ext["ospans"].tolist(),
                    oflags=ext["oflags"].tolist(), recs=fresh.verify_emails(emails))
    finally:
        fresh.close()
    # the inputs do what they are there for: signatures found, keys decoded, a body in its second place, a selection made, strings captured
    assert [len(x.sigs) for x in want["scan"]] == [1, 1, 1, 0, 0] and [k.code for k in want["keyrec"][:3]] == [0, 0, 0]
    assert [want["bodies"][k].body for k in (3, 4)] == [body_model.verdict(raws[k], False)[1].data for k in (3, 4)]
    assert want["bodies"][3].body.startswith(b"a\r\nb\r\n\r\nc") and len(want["bodies"][4].body) > len(outgrows)
    assert want["sel_chosen"][:3] == [1, 0, A.SEL_NONE] and [int(x) for x in want["recs"]["status"][:3]] == [A.ZKE_OK] * 3
    assert int(ext["out"][0]["status"]) == A.ZKE_OK and (ext["spans"][:4] != QM.NO).all()

    for slots, reverse in ((1, False), (2, True)):
        eng = z.Engine(slots=slots)
        try:
            tickets, outputs = submit_all(eng, QM.parts_of(eng, patterns))
            for t in (reversed(tickets) if reverse else tickets):
                assert eng.lib.zke_batch_wait(eng.h, t) == 0, (slots, t)
            got = outputs()
            for k in ("scan", "keyrec", "bodies", "sel_chosen", "sel_keys", "ext", "ospans", "oflags"):
                assert got[k] == want[k], (slots, k)
            assert_records_equal(got["sel_out"], want["sel_out"], None, f"selection, {slots} slot(s)")
            assert_records_equal(got["recs"], want["recs"], None, f"verify, {slots} slot(s)")
        finally:
            eng.close()


def _capture_mixed(eng, refs, lists, ticket):
    """zke_extract_captures_mixed[_async] with origins through the C entry, into buffers sized once (64 bytes of blob per column)."""
    n, J, Gt = refs.n, lists.J, lists.Gt
    st = dict(out=np.zeros(max(n, 1), dtype=A.RESULT_DTYPE), spans=np.zeros(max(Gt * 2, 1), np.uint32), flags=np.zeros(max(Gt, 1), np.uint8),
              cap_off=np.zeros(J + 1, np.uint32), cap_str_off=np.zeros(Gt + 1, np.uint32), blob=np.zeros(max(64 * Gt, 1), np.uint8),
              ospans=np.full(max(Gt * 2, 1), 0x55555555, np.uint32), oflags=np.full(max(Gt, 1), 0x55, np.uint8), keep=(refs, lists))
    o, org = A.zke_capture_out(), A.zke_capture_origin()
    o.spans, o.spans_cap, o.flags, o.flags_cap = st["spans"].ctypes.data, Gt * 2, st["flags"].ctypes.data, Gt
    o.cap_off, o.cap_off_cap, o.cap_str_off, o.cap_str_off_cap = st["cap_off"].ctypes.data, J + 1, st["cap_str_off"].ctypes.data, Gt + 1
    o.cap_blob, o.cap_blob_cap = st["blob"].ctypes.data, 64 * Gt
    org.spans, org.spans_cap, org.flags, org.flags_cap = st["ospans"].ctypes.data, Gt * 2, st["oflags"].ctypes.data, Gt
    st["o"], st["org"], st["ticket"] = o, org, C.c_uint64()
    args = [eng.h, refs.arr, n, C.byref(lists.c), st["out"].ctypes.data, C.byref(o), C.byref(org)]
    name = "zke_extract_captures_mixed" + ("_async" if ticket else "")
    assert getattr(eng.lib, name)(*(args + ([C.byref(st["ticket"])] if ticket else []))) == 0, eng.lib.zke_last_error(None)
    st["read"] = lambda: dict(out=st["out"][:n].tobytes(), spans=st["spans"][:Gt * 2].tolist(), flags=st["flags"][:Gt].tolist(), cap_off=st["cap_off"].tolist(),
                              cap_str_off=st["cap_str_off"][:int(o.n_strings) + 1].tolist(), blob=st["blob"][:int(o.cap_blob_need)].tobytes(),
                              ospans=st["ospans"][:Gt * 2].tolist(), oflags=st["oflags"][:Gt].tolist())
    return st


def test_every_plan_section_in_turn_on_one_slot():
    """Every kind of plan section through ONE slot, one after the other, none waited for: a mixed verify (the mixed plan), a mixed
    extraction with origins through the C entry (the plan and the extraction's tables), a plain verify — an image without a plan
    section behind two with —, an encoded mixed verify (the plan and a host-planned encoding) and an extraction with a device-planned
    encoding — each retired by the submission behind it, the last by its wait.  Every output equals what the synchronous entry
    returns for the same call on a fresh engine.  Then the same sequence through two slots, waited for in reverse order.  A section
    staged at the wrong offset of the image, or viewed from a stale one, shows here as wrong bytes.  Five e-mails of the case list,
    the three signed ones in front; two regex configs and one e-mail without; every other e-mail has an external input."""
    import dataclasses
    import zkemail_rs_amd as z
    from zkemail_rs_amd import regex_compile as rc
    every = cases.build_cases()
    good = [x for x in every if x.status == A.ZKE_OK and x.email.public_key.key_type == "rsa"][:3]
    more = [x for x in every if all(x is not g for g in good)][:2]
    assert len(good) == 3 and len(more) == 2
    emails = [dataclasses.replace(x.email, external_inputs=[A.ExternalInput("order", "no-%d" % i, 16)] if i % 2 == 0 else [])
              for i, x in enumerate(good + more)]
    P = rc.RegexPattern
    subject = P(*synth.HEADER_PATTERNS[1])
    cfg_a, cfg_b = rc.RegexConfig([subject], [P(*_body_word_pattern(good[0]))]), rc.RegexConfig([subject], None)
    configs = [cfg_a, cfg_b, None, cfg_a, cfg_b]
    roomy = dict(unicode=False, blob_bytes=1 << 12, bytes_cap=1 << 14)

    fresh = z.Engine()
    try:
        # the inputs of the verify entries: every e-mail with the RegexInfo its config extracts from it ("?" where it extracts nothing)
        _, found = fresh.extract_captures_mixed(emails, configs, unicode=False)
        def info(cfg, got):
            side = lambda parts: None if parts is None else [A.CompiledRegex(fresh.compile_pattern(p.pattern, False)[0], ["?"] * len(p.capture_indices or []))
                                                               for p in parts]
            return got if got is not None else A.RegexInfo(side(cfg.header_parts), side(cfg.body_parts))
        inputs = [e if cfg is None else A.EmailWithRegex(e, info(cfg, got)) for e, cfg, got in zip(emails, configs, found)]
        xe = fresh.extract_captures_encoded_call(emails, cfg_b, **roomy)
        assert xe.rc == 0
        enc = fresh.verify_emails_encoded(inputs, form="mixed")
        want = dict(mixed=fresh.verify_emails_mixed(inputs), capmix=_capture_mixed(fresh, A.EmailRefs(emails), fresh.pack_capture_mixed(configs, unicode=False)[0], False)["read"](),
                    plain=fresh.verify_emails(emails), enc_recs=enc[0], enc=enc[1], xe_recs=xe.records, xe=xe.enc.result(), xe_strings=xe.strings(),
                    xe_needs=(int(xe.caps.cap_blob_need), int(xe.enc.c.bytes_need)))
    finally:
        fresh.close()
    # the inputs do what they are there for: an e-mail with a config and the one without verify, strings are captured, encodings come out
    assert [int(want["mixed"]["status"][i]) for i in (0, 2)] == [A.ZKE_OK] * 2 and [int(s) for s in want["plain"]["status"][:3]] == [A.ZKE_OK] * 3
    assert found[0] is not None and len(found[0].body_parts[0].captures) == 1 and found[2] is None
    assert all(len(want[k][0][0]) > 0 for k in ("enc", "xe")) and len(want["enc"][2][0]) > 0 and len(want["xe_strings"][0]) == 1

    for slots, reverse in ((1, False), (2, True)):
        eng = z.Engine(slots=slots)
        try:
            lists = eng.pack_capture_mixed(configs, unicode=False)[0]
            t1, mixed = eng.verify_emails_mixed_async(inputs)
            capmix = _capture_mixed(eng, A.EmailRefs(emails), lists, True)
            refs = A.EmailRefs(emails)
            t3, plain = eng.verify_emails_async(refs)
            t4, enc = eng.verify_emails_encoded_async(inputs, form="mixed")
            xe = eng.extract_captures_encoded_call(emails, cfg_b, ticket=True, **roomy)
            assert xe.rc == 0
            tickets = [t1, capmix["ticket"].value, t3, t4, xe.ticket]
            for t in (reversed(tickets) if reverse else tickets):
                assert eng.lib.zke_batch_wait(eng.h, t) == 0, (slots, t)
            assert_records_equal(mixed, want["mixed"], None, f"mixed verify, {slots} slot(s)")
            assert capmix["read"]() == want["capmix"], slots
            assert_records_equal(plain, want["plain"], None, f"plain verify, {slots} slot(s)")
            assert_records_equal(enc.records, want["enc_recs"], None, f"encoded verify, {slots} slot(s)")
            assert enc.enc.result() == want["enc"], slots
            assert_records_equal(xe.records, want["xe_recs"], None, f"encoded extraction, {slots} slot(s)")
            assert xe.enc.result() == want["xe"] and xe.strings() == want["xe_strings"], slots
            assert (int(xe.caps.cap_blob_need), int(xe.enc.c.bytes_need)) == want["xe_needs"], slots
        finally:
            eng.close()
