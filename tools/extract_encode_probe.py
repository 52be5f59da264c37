"""Time zke_extract_captures_encoded against the two-call path it replaces (not bench.py: nothing here is a threshold).  One batch:

  c3   BASELINE configs[2]'s shape: 4 096 DKIM-signed e-mails, 4 KB of body, RSA-2048, 2 header parts with one capture each

Two ways from raw e-mails, keys and a part list to {records, capture tables, encodings, digests}, interleaved round by round after a
warm-up, each synchronous (the device is idle when the clock stops), every argument built outside the clock:

  (a) zke_extract_captures_encoded      one call: one upload, one pipeline, the repair and the plan on the device
  (b) zke_extract_captures              the tables come back as raw bytes,
      + the host repair                 the strings flagged ZKE_CAPF_NOT_UTF8 are repaired in Python and the tables rebuilt (this
                                        batch's subjects and addresses are ASCII: the step is the look at the flags),
      + zke_verify_emails_encoded       the same e-mails uploaded again with the tables: front end, hash / modexp, regex, encode, hash

Every round of (a) is compared with (b)'s product first.  The whole measurement is repeated `--runs` times in one process; the
medians of the runs and their spread are what the file reports.

    python tools/extract_encode_probe.py --out profiles/extract_encode_probe.txt
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def med(xs):
    xs = sorted(xs)
    return statistics.median(xs), xs[len(xs) // 10], xs[-(len(xs) // 10) - 1]


def fmt(t):
    return f"{t[0]:9.1f} us [{t[1]:.1f} .. {t[2]:.1f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import synth
    import zkemail_rs_amd as z
    from zkemail_rs_amd import _abi as A
    from zkemail_rs_amd import regex_compile as rc

    eng = z.Engine()
    n = args.n
    inputs, _, _ = synth.make_regex_workload("c3", n, 4096, rsa_bits=2048, n_keys=16, seed=4243, n_header_parts=2, n_body_parts=0)
    emails = [i.email for i in inputs]
    cfg = rc.RegexConfig([rc.RegexPattern(p, ci) for p, ci in synth.HEADER_PATTERNS[:2]], None)
    # (a): one call builds every argument (and runs once); the timed calls repeat the C entry with them
    a = eng.extract_captures_encoded_call(emails, cfg, unicode=False, blob_bytes=64 * n * 2, bytes_cap=1024 * n)
    assert a.rc == 0, eng.lib.zke_last_error(None)
    refs, arr, groups, ext = a.keep
    P, G = a.P, a.G
    gbase = [sum(len(g) for g in groups[:p]) for p in range(P)]
    # (b): the extraction's buffers, and a zke_encode_in whose lists point at them
    out_b = np.zeros(n, A.RESULT_DTYPE)
    spans, flags = np.zeros(n * G * 2, np.uint32), np.zeros(n * G, np.uint8)
    cap_off, cap_str_off, blob = np.zeros(n * P + 1, np.uint32), np.zeros(n * G + 1, np.uint32), np.zeros(64 * n * G, np.uint8)
    o = A.zke_capture_out()
    o.spans, o.spans_cap, o.flags, o.flags_cap = spans.ctypes.data, n * G * 2, flags.ctypes.data, n * G
    o.cap_off, o.cap_off_cap, o.cap_str_off, o.cap_str_off_cap = cap_off.ctypes.data, n * P + 1, cap_str_off.ctypes.data, n * G + 1
    o.cap_blob, o.cap_blob_cap = blob.ctypes.data, blob.size
    ids = np.array([c[1] for c in a.comp], np.uint32)
    lists = A.zke_regex_lists()
    lists.n_header_parts, lists.header_part_ids, lists.n_body_parts, lists.body_part_ids = P, ids.ctypes.data, 0, None
    enc_in = A.zke_encode_in()
    enc_in.lists = C.pointer(lists)
    if ext.n_strings:
        enc_in.ext_off, enc_in.ext_str_off, enc_in.ext_blob = ext.off.ctypes.data, ext.str_off.ctypes.data, ext.blob.ctypes.data
    rec_b = np.zeros(n, A.RESULT_DTYPE)
    enc_b = A.EncodedBuffers(n, 1024 * n)
    keep = []

    def run_a():
        rcode = eng.lib.zke_extract_captures_encoded(*a.args)
        assert rcode == 0, rcode

    def run_b():
        rcode = eng.lib.zke_extract_captures(eng.h, refs.arr, n, arr, P, None, 0, out_b.ctypes.data, C.byref(o))
        assert rcode == 0, rcode
        so, bl = cap_str_off, blob
        if flags.any():                          # helpers/src/regex.rs:35 on the host: the flagged strings, then the tables again
            raw, fixed = blob.tobytes(), []
            for i in range(n):
                for p in range(P):
                    k0 = int(cap_off[i * P + p])
                    for k in range(k0, int(cap_off[i * P + p + 1])):      # string k is column gbase[p] + (k - k0) of e-mail i
                        s = raw[int(cap_str_off[k]):int(cap_str_off[k + 1])]
                        bad = flags[i * G + gbase[p] + (k - k0)] & A.CAPF_NOT_UTF8
                        fixed.append(s.decode("utf-8", "replace").encode() if bad else s)
            tb = A.StringTable([fixed])
            so, bl = tb.str_off, tb.blob
            keep[:] = [tb]
        lists.cap_off, lists.cap_str_off, lists.cap_blob = cap_off.ctypes.data, so.ctypes.data, bl.ctypes.data
        rcode = eng.lib.zke_verify_emails_encoded(eng.h, refs.arr, n, C.byref(enc_in), rec_b.ctypes.data, C.byref(enc_b.c))
        assert rcode == 0, (rcode, eng.lib.zke_last_error(None))

    runs = []
    for _ in range(args.runs):
        ta, tb_ = [], []
        for k in range(args.warmup + args.steps):
            t0 = time.perf_counter(); run_a(); t1 = time.perf_counter()
            run_b(); t2 = time.perf_counter()
            assert a.records.tobytes() == out_b.tobytes() == rec_b.tobytes(), "(a) and (b) give the same records"
            assert a.enc.result() == enc_b.result(), "(a) and (b) give the same encodings and digests"
            if k >= args.warmup:
                ta.append((t1 - t0) * 1e6); tb_.append((t2 - t1) * 1e6)
        runs.append((med(ta), med(tb_)))
    ok = int((a.records["status"] == 0).sum())
    ma, mb = [r[0][0] for r in runs], [r[1][0] for r in runs]
    lines = [f"extract_encode_probe: steps={args.steps} warmup={args.warmup} runs={args.runs} (one engine, one slot; per run the median [10th .. 90th "
             "percentile]; host clock around synchronous calls, (a) and (b) alternating)",
             f"c3: {n} e-mails, 4 KB bodies, RSA-2048, 2 header parts with one capture each; {ok} of {n} encoded, "
             f"{int(a.enc.c.bytes_need) / n:.0f} B of encoding and {int(a.caps.cap_blob_need) / n:.1f} B of strings per e-mail"]
    for k, (xa, xb) in enumerate(runs):
        lines.append(f"    run {k}: (a) {fmt(xa)}    (b) {fmt(xb)}    (b) / (a) = {xb[0] / xa[0]:.2f}")
    lines.append(f"    medians of the runs: (a) {statistics.median(ma):.1f} us (spread {min(ma):.1f} .. {max(ma):.1f}), "
                 f"(b) {statistics.median(mb):.1f} us (spread {min(mb):.1f} .. {max(mb):.1f}); (b) / (a) = {statistics.median(mb) / statistics.median(ma):.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
