#!/usr/bin/env python
"""queue_trace.py DIR [STEP_MS]: how a rocprofv3 --kernel-trace run of bench.py used the hardware queues.

Reads DIR/**/*_kernel_trace.csv.  Per queue: launches, busy time (sum of kernel durations), the span from its first start to its
last end, and how much consecutive kernels of that queue overlap (a hardware queue runs its packets one after the other: the
overlap must be ~0).  Then the steady-state figures the throughput model of DESIGN.md §5 rests on: batches (one verdict kernel
each) per queue, busy time per batch, and span / batches over all queues = the step the chain would give.
"""
import csv
import glob
import os
import sys
from collections import defaultdict


def short(name: str) -> str:
    name = name.split("(")[0]
    for pre in ("void ", "zke::"):
        name = name.replace(pre, "")
    return name[:40]


def check_map(d: str, probe_log: str):
    """queue_trace.py DIR --map PROBE_LOG: the hardware queue each slot's kernels ran on, from the trace, against the group the engine
    reported for the slot (the `queue_probe slot K group G HW_ID by XCC: ...` lines a -DZKE_DEV_KNOBS build prints under
    ZKE_DEBUG_QUEUE_PROBE=1).  zke_engine_reserve launches one slot_queue_probe_kernel per slot, in slot order: the k-th of them by
    dispatch id is slot k's, and its Queue_Id is the slot stream's queue."""
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                if "slot_queue_probe_kernel" in r["Kernel_Name"]:
                    rows.append((int(r.get("Dispatch_Id") or r["Start_Timestamp"]), r["Queue_Id"]))
    rows.sort()
    groups, words = {}, {}
    for line in open(probe_log):
        if line.startswith("queue_probe slot"):
            p = line.split()
            groups[int(p[2])], words[int(p[2])] = int(p[4]), p[8:]
    S = len(groups)
    if not S or len(rows) < S:
        raise SystemExit(f"{S} slots in the probe log, {len(rows)} probe launches in the trace")
    traced = [q for _, q in rows[-S:]]          # the last reserve's
    print("slot  trace_queue  engine_group  HW_ID by XCC 0..7")
    for s in range(S):
        print(f"{s:4d}  {traced[s]:>11}  {groups[s]:12d}  {' '.join(words[s])}")
    same_t = [[traced[a] == traced[b] for b in range(S)] for a in range(S)]
    same_e = [[groups[a] == groups[b] and groups[a] >= 0 for b in range(S)] for a in range(S)]
    ok = same_t == same_e
    print(f"trace queues {len(set(traced))}, engine groups {len(set(groups.values()))}: the partitions are {'IDENTICAL' if ok else 'DIFFERENT'}")
    sys.exit(0 if ok else 1)


def main():
    d = sys.argv[1]
    if len(sys.argv) > 3 and sys.argv[2] == "--map":
        return check_map(d, sys.argv[3])
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {d}")
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                rows.append((r["Queue_Id"], int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
    by_q = defaultdict(list)
    for q, s, e, n in rows:
        by_q[q].append((s, e, n))
    # steady state: the last 60 % of the batches of the trace (warm-up, priming and the alone pass come first)
    verdict_ends = sorted(e for _, _, e, n in rows if n.startswith("ed_verdict"))
    if len(verdict_ends) < 20:
        raise SystemExit("fewer than 20 verdict kernels in the trace")
    t_lo, t_hi = verdict_ends[int(len(verdict_ends) * 0.4)], verdict_ends[-1]
    print(f"{len(rows)} kernels on {len(by_q)} queues; steady window {1e-6 * (t_hi - t_lo):.3f} ms")
    tot_batches = 0
    print("queue  kernels  batches  busy_us/batch  span_us/batch  overlap_us(max)  overlapping_pairs  kernels_us(mean in window)")
    for q in sorted(by_q):
        ks = sorted(k for k in by_q[q] if t_lo <= k[0] and k[1] <= t_hi)
        if not ks:
            print(f"{q:>5}  (idle in the window)")
            continue
        busy = sum(e - s for s, e, _ in ks)
        span = ks[-1][1] - ks[0][0]
        nb = sum(1 for k in ks if k[2].startswith("ed_verdict"))
        ov = [ks[i][1] - ks[i + 1][0] for i in range(len(ks) - 1) if ks[i][1] > ks[i + 1][0]]
        per = defaultdict(list)
        for s, e, n in ks:
            per[n].append(e - s)
        means = ", ".join(f"{n} {1e-3 * sum(v) / len(v):.1f}" for n, v in sorted(per.items(), key=lambda kv: -sum(kv[1])))
        tot_batches += nb
        if nb:
            print(f"{q:>5}  {len(ks):7d}  {nb:7d}  {1e-3 * busy / nb:13.1f}  {1e-3 * span / nb:13.1f}  {1e-3 * max(ov, default=0):15.2f}  {len(ov):17d}  {means}")
        else:
            print(f"{q:>5}  {len(ks):7d}  {nb:7d}  (no batches)  {means}")
    step_us = 1e-3 * (t_hi - t_lo) / max(1, tot_batches)
    print(f"batches in window {tot_batches}; step from the trace {step_us:.1f} us")
    # how many kernels of DIFFERENT queues run at the same time, averaged over the window
    ev = []
    for q, s, e, n in rows:
        if t_lo <= s and e <= t_hi:
            ev += [(s, 1), (e, -1)]
    ev.sort()
    cur, last, acc = 0, t_lo, 0
    for t, dlt in ev:
        acc += cur * (t - last)
        cur, last = cur + dlt, t
    print(f"kernels running at once, time average {acc / (t_hi - t_lo):.2f}")
    if len(sys.argv) > 2:
        print(f"bench step {float(sys.argv[2]) * 1e3:.1f} us")


if __name__ == "__main__":
    main()
