"""Time one mixed regex batch against what a caller had to do without it (not bench.py: nothing here is a threshold).

4 096 e-mails of the BASELINE configs[2] shape (4 KB bodies, RSA-2048, two header parts per config) spread evenly over K = 1, 2, 4, 8,
16 regex configs — K distinct ordered pairs of header patterns.  Three routes, interleaved round by round on one engine with 16 slots:

  (a) the route without zke_verify_emails_mixed: the queue sorted by config, K asynchronous zke_verify_emails_with_regex calls of
      n / K e-mails each on K slots, then K waits;
  (b) ONE zke_verify_emails_mixed call over the queue as it stands (configs interleaved i % K);
  (c) K = 1 only: zke_verify_emails_with_regex over the whole batch — what the segment lookup and the permutation cost.

Every figure is the host clock around the C calls, from the first submission to the last wait (the calls end in the wait for the
records: nothing is still in flight when the clock stops); the tables are packed beforehand.  Before anything is timed the records of
(a), (b) and (c) are compared: they must be equal.  The e-mails are 256 signed ones repeated.

The acceptance on record: (b) is not slower than (a) beyond (a)'s own round-to-round spread for K >= 2; the K = 1 difference between
(b) and (c) is reported as it comes out.

    python tools/mixed_regex_probe.py --out profiles/mixed_regex_probe.txt
"""
import argparse
import ctypes as C
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PATTERNS = [                       # each matches exactly once in the canonical header block of a synth e-mail
    (r"from:[^\r\n]*<([a-z]+)@example\.com>\r\n", [1]), (r"subject:([^\r\n]+)\r\n", [1]), (r"to:([^\r\n]+)\r\n", [1]),
    (r"date:([^\r\n]+)\r\n", [1]), (r"message-id:<([^>]+)>", [1]), (r"subject:[^\r\n]+\r\n", []), (r"from:[^\r\n]*@example\.com", []),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--distinct", type=int, default=256)
    ap.add_argument("--body", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import synth
    import zkemail_rs_amd as z
    from zkemail_rs_amd import _abi as A
    from zkemail_rs_amd import regex_compile as rc

    n = args.n
    base, wl, _ = synth.make_regex_workload("c3", args.distinct, args.body, rsa_bits=2048, n_keys=16, seed=3, n_header_parts=2)
    dfas = [rc.create_dfa(p) for p, _ in PATTERNS]
    pairs = [(a, b) for a in range(len(PATTERNS)) for b in range(len(PATTERNS)) if a != b][:16]

    def with_config(k, cfg):
        it = wl.inter[k % args.distinct]
        parts = []
        for ix in pairs[cfg]:
            m = re.search(PATTERNS[ix][0].encode(), it["canon_header"])
            parts.append(A.CompiledRegex(dfas[ix], [m.group(g).decode() for g in PATTERNS[ix][1]]))
        return A.EmailWithRegex(base[k % args.distinct].email, A.RegexInfo(parts, None))

    eng = z.Engine(slots=16)
    eng.reserve(n, n * (args.body + 2048), 16, 2)
    lib = eng.lib

    def lists_of(p):
        ls = A.zke_regex_lists()
        ls.n_header_parts, ls.n_body_parts = p.nh, p.nb
        ls.header_part_ids, ls.body_part_ids = p.hdr_ids.ctypes.data, p.body_ids.ctypes.data
        ls.cap_off, ls.cap_str_off, ls.cap_blob = p.cap_off.ctypes.data, p.cap_str_off.ctypes.data, p.cap_blob.ctypes.data
        return ls

    lines = [f"mixed_regex_probe: rounds={args.rounds} warmup={args.warmup} n={n} ({args.distinct} distinct e-mails repeated), "
             f"{args.body} B bodies, two header parts per config, 16 slots; host clock, first submission to last wait, microseconds: "
             "median [min .. max] over the rounds"]
    for K in (1, 2, 4, 8, 16):
        queue = [with_config(i, i % K) for i in range(n)]                     # the queue as it stands: configs interleaved
        ml, mrefs = eng.pack_mixed(queue), A.EmailRefs([q.email for q in queue])
        mout = np.zeros(n, dtype=A.RESULT_DTYPE)
        groups = []                                                           # (a): the queue sorted by config
        for c in range(K):
            idx = [i for i in range(n) if i % K == c]
            sub = [queue[i] for i in idx]
            p = eng.pack_with_regex(sub)
            groups.append((idx, p, lists_of(p), A.EmailRefs([q.email for q in sub]), np.zeros(len(sub), dtype=A.RESULT_DTYPE), C.c_uint64()))

        def route_a():
            for idx, p, ls, refs, out, t in groups:
                rc_ = lib.zke_verify_emails_with_regex_async(eng.h, refs.arr, refs.n, C.byref(ls), out.ctypes.data, C.byref(t))
                assert rc_ == 0, rc_
            for g in groups:
                assert lib.zke_batch_wait(eng.h, g[5].value) == 0

        def route_b():
            assert lib.zke_verify_emails_mixed(eng.h, mrefs.arr, n, C.byref(ml.c), mout.ctypes.data) == 0

        def route_c():
            idx, p, ls, refs, out, t = groups[0]
            assert lib.zke_verify_emails_with_regex(eng.h, refs.arr, refs.n, C.byref(ls), out.ctypes.data) == 0

        routes = [("a", route_a), ("b", route_b)] + ([("c", route_c)] if K == 1 else [])
        route_a()
        route_b()
        for idx, p, ls, refs, out, t in groups:                                # the records of the routes are the same
            for f in A.RESULT_DTYPE.names:
                assert (out[f] == mout[idx][f]).all(), (K, f)
        assert int((mout["status"] == 0).sum()) == n
        times = {name: [] for name, _ in routes}
        for r in range(args.warmup + args.rounds):
            for name, call in routes:
                t0 = time.perf_counter()
                call()
                dt = (time.perf_counter() - t0) * 1e6
                if r >= args.warmup:
                    times[name].append(dt)
        stat = {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}
        row = f"  K={K:2d}  " + "   ".join(f"({k}) {s[0]:8.1f} [{s[1]:.1f} .. {s[2]:.1f}]" for k, s in stat.items())
        a, b = stat["a"], stat["b"]
        row += f"   (b) - (a) = {b[0] - a[0]:+.1f} us, (a)'s spread {a[2] - a[1]:.1f} us"
        if K == 1:
            row += f"; (b) - (c) = {b[0] - stat['c'][0]:+.1f} us"
        lines.append(row)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
