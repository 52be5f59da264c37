"""Time one mixed extraction against what a caller had to do without it (not bench.py: nothing here is a threshold).

4 096 e-mails of the BASELINE configs[2] shape (4 KB bodies, RSA-2048, two header parts per config, one group each) spread evenly over
K = 1, 2, 4, 8, 16 regex configs — K distinct ordered pairs of header patterns.  Routes, interleaved round by round on one engine with
16 slots:

  (a) the route without zke_extract_captures_mixed, the yardstick: the queue sorted by config, K asynchronous zke_extract_captures
      calls of n / K e-mails each on K slots, then K waits (the re-interleaving of the K ragged tables into the e-mail-major layout
      zke_regex_mixed takes, which that caller also owes, is NOT timed);
  (b) ONE zke_extract_captures_mixed call over the queue as it stands (configs interleaved i % K);
  (c) K = 1 only: zke_extract_captures over the whole batch — what the ragged lookups cost.

Every figure is the host clock around the C calls, from the first submission to the last wait (the calls end in the wait for the
records and tables: nothing is in flight when the clock stops); the tables are packed and every buffer allocated beforehand.  Before
anything is timed the records and strings of the routes are compared: they must be equal.  The e-mails are 256 signed ones repeated.

    python tools/capture_mixed_probe.py --out profiles/capture_mixed_probe.txt
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PATTERNS = [                       # each matches exactly once in the canonical header block of a synth e-mail
    (r"from:[^\r\n]*<([a-z]+)@example\.com>\r\n", [1]), (r"subject:([^\r\n]+)\r\n", [1]), (r"to:([^\r\n]+)\r\n", [1]),
    (r"date:([^\r\n]+)\r\n", [1]), (r"message-id:<([^>]+)>", [1]), (r"subject:([^\r\n]+)\r\n", [0]), (r"from:[^\r\n]*@(example\.com)", [1]),
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

    n = args.n
    base, wl, _ = synth.make_regex_workload("c3", args.distinct, args.body, rsa_bits=2048, n_keys=16, seed=3, n_header_parts=2)
    emails = [base[k % args.distinct].email for k in range(n)]
    pairs = [(a, b) for a in range(len(PATTERNS)) for b in range(len(PATTERNS)) if a != b][:16]

    eng = z.Engine(slots=16)
    eng.reserve(n, n * (args.body + 2048), 16, 2)
    lib = eng.lib
    parts = [(*eng.compile_pattern(p, False)[1:], g) for p, g in PATTERNS]

    class Bufs:
        """A zke_capture_out with buffers for J jobs and Gt columns, 256 bytes of blob per column."""
        def __init__(self, m, J, Gt):
            self.out = np.zeros(max(m, 1), dtype=A.RESULT_DTYPE)
            self.spans, self.flags = np.zeros(max(2 * Gt, 1), np.uint32), np.zeros(max(Gt, 1), np.uint8)
            self.cap_off, self.cap_str_off, self.blob = np.zeros(J + 1, np.uint32), np.zeros(Gt + 1, np.uint32), np.zeros(256 * Gt + 1, np.uint8)
            o = self.o = A.zke_capture_out()
            o.spans, o.spans_cap, o.flags, o.flags_cap = self.spans.ctypes.data, 2 * Gt, self.flags.ctypes.data, Gt
            o.cap_off, o.cap_off_cap, o.cap_str_off, o.cap_str_off_cap = self.cap_off.ctypes.data, J + 1, self.cap_str_off.ctypes.data, Gt + 1
            o.cap_blob, o.cap_blob_cap = self.blob.ctypes.data, 256 * Gt
            self.ticket = C.c_uint64()

        def strings(self):
            raw = self.blob.tobytes()
            return [raw[self.cap_str_off[k]:self.cap_str_off[k + 1]] for k in range(int(self.o.n_strings))]

    lines = [f"capture_mixed_probe: rounds={args.rounds} warmup={args.warmup} n={n} ({args.distinct} distinct e-mails repeated), "
             f"{args.body} B bodies, two header parts of one group per config, 16 slots; host clock, first submission to last wait, "
             "microseconds: median [min .. max] over the rounds"]
    for K in (1, 2, 4, 8, 16):
        configs = [([parts[a], parts[b]], []) for a, b in pairs[:K]]
        lists = A.CaptureMixedLists(configs, [i % K for i in range(n)])          # the queue as it stands: configs interleaved
        mrefs, mb = A.EmailRefs(emails), Bufs(n, lists.J, lists.Gt)
        groups = []                                                              # (a): the queue sorted by config
        for c in range(K):
            idx = [i for i in range(n) if i % K == c]
            one = A.CaptureMixedLists([configs[c]], [0] * len(idx))              # (its part array is what the single-config entry takes)
            groups.append((idx, one, A.EmailRefs([emails[i] for i in idx]), Bufs(len(idx), 2 * len(idx), 2 * len(idx))))

        def route_a():
            for idx, one, refs, b in groups:
                cf = one.arr[0]
                rc_ = lib.zke_extract_captures_async(eng.h, refs.arr, refs.n, cf.header_parts, 2, cf.body_parts, 0, b.out.ctypes.data, C.byref(b.o),
                                                     C.byref(b.ticket))
                assert rc_ == 0, rc_
            for g in groups:
                assert lib.zke_batch_wait(eng.h, g[3].ticket.value) == 0

        def route_b():
            assert lib.zke_extract_captures_mixed(eng.h, mrefs.arr, n, C.byref(lists.c), mb.out.ctypes.data, C.byref(mb.o), None) == 0

        def route_c():
            idx, one, refs, b = groups[0]
            cf = one.arr[0]
            assert lib.zke_extract_captures(eng.h, refs.arr, refs.n, cf.header_parts, 2, cf.body_parts, 0, b.out.ctypes.data, C.byref(b.o)) == 0

        routes = [("a", route_a), ("b", route_b)] + ([("c", route_c)] if K == 1 else [])
        route_a()
        route_b()
        mstr = mb.strings()
        assert int((mb.out["status"] == 0).sum()) == n and len(mstr) == 2 * n
        for idx, one, refs, b in groups:                                          # the records and strings of the routes are the same
            for f in A.RESULT_DTYPE.names:
                if f != "reserved":
                    assert (b.out[f] == mb.out[idx][f]).all(), (K, f)
            assert b.strings() == [s for i in idx for s in mstr[2 * i:2 * i + 2]], K
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
