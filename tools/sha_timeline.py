#!/usr/bin/env python
"""sha_timeline.py [--reps K] [--plain] [--keep FILE]: where the waves of the two-role SHA-256 routines run and what a block costs them.

Builds tests/cpp/sha_probe (build.build_sha_probe: csrc/sha256.hip.h compiled with ZKE_SHA_PROBE) and runs it ONCE, under a time
limit: sha256_pair_kernel and sha256_ring_kernel alone on 1 024 messages of 4 KB.  Prints
  * each kernel's median time, per block in us and in clock ticks of the stamps (s_memtime), and whether its digests are hashlib's;
  * where the waves of every workgroup landed (SIMD, CU, SE, XCC from HW_ID / XCC_ID), for the two kernels and for plain
    workgroups of 128, 192 and 256 threads, and how many workgroups have two waves on one SIMD;
  * for blocks 8..15 of group 0, per wave: the time between the stamps (the work) and the time spent at each barrier.
--plain runs the build without stamps (the code the library runs) for the times alone.  profiles/sha_ring_timeline.txt is this
program's output."""
import argparse
import collections
import hashlib
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, LEN, BLOCKS = 1024, 4096, 65
POINTS = {"pair": ["loop top", "reads issued (feeder: nothing)", "after barrier 1", "work done", "after barrier 2"],
          "ring": ["loop top", "work done", "after the barrier"]}


def message(i):
    return bytes((131 * i + 7 * j + (j >> 8)) & 255 for j in range(LEN))


def where(hw, xcc):
    return {"simd": (hw >> 4) & 3, "cu": (hw >> 8) & 15, "sh": (hw >> 12) & 1, "se": (hw >> 13) & 7, "xcc": xcc & 15}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--keep", help="keep the probe's report in this file")
    ap.add_argument("--timeout", type=int, default=120)
    args = ap.parse_args()
    from zkemail_rs_amd import build
    exe = build.build_sha_probe(stamps=not args.plain)
    with tempfile.TemporaryDirectory() as d:
        path = args.keep or os.path.join(d, "report.txt")
        r = subprocess.run([exe, path, str(args.reps)], timeout=args.timeout, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            raise SystemExit("sha_probe exited with %d" % r.returncode)
        lines = [ln.split() for ln in open(path)]
    times = {ln[1]: (float(ln[2]), float(ln[3])) for ln in lines if ln[0] == "time"}
    stamps = collections.defaultdict(dict)
    for ln in lines:
        if ln[0] == "stamp":
            stamps[(ln[1], int(ln[2]), int(ln[3]))][int(ln[4])] = int(ln[5])
    print("build: %s" % ("without stamps" if args.plain else "with stamps (ZKE_SHA_PROBE): the stamps cost time themselves"))
    for k, (med, lo) in times.items():
        print(f"{k}: median {med:.1f} us, best {lo:.1f} us over {args.reps} launches; {med / BLOCKS:.3f} us per block")
    for ln in lines:
        if ln[0] == "digest":
            ok = hashlib.sha256(message(int(ln[2]))).hexdigest() == ln[3]
            print(f"digest {ln[1]} message {ln[2]}: {'hashlib' if ok else 'WRONG'}")
            if not ok:
                raise SystemExit(1)
    print()
    print("placement (one line per workgroup: simd of wave 0, 1, ... | cu se xcc of wave 0; * = two waves of it on one SIMD)")
    groups = collections.defaultdict(dict)
    for ln in lines:
        if ln[0] == "where":
            groups[(ln[1], int(ln[2]))][int(ln[3])] = where(int(ln[4], 16), int(ln[5], 16))
    shared = collections.Counter()
    total = collections.Counter()
    split_cu = collections.Counter()
    for (k, g), waves in sorted(groups.items()):
        simds = [waves[w]["simd"] for w in sorted(waves)]
        same = len(set(simds)) < len(simds)
        other_cu = len({(w["cu"], w["sh"], w["se"], w["xcc"]) for w in waves.values()}) > 1
        total[k] += 1
        shared[k] += same
        split_cu[k] += other_cu
        w0 = waves[0]
        print(f"  {k:6s} group {g:2d}: simd {' '.join(map(str, simds))} | cu {w0['cu']:2d} se {w0['se']} xcc {w0['xcc']}{' *' if same else ''}{' (waves on different CUs?)' if other_cu else ''}")
    for k in total:
        print(f"  {k}: {shared[k]} of {total[k]} workgroups have two waves on one SIMD")
    if stamps:
        print()
        print("group 0, blocks 8..15, clock ticks between consecutive stamps (role 0 feeder, 1 rounds)")
        for k in ("pair", "ring"):
            names = POINTS[k]
            print(f"  {k}: " + " -> ".join(names))
            per_block = []
            for role in (0, 1):
                for blk in range(8, 16):
                    s = stamps.get((k, role, blk))
                    if not s:
                        continue
                    d = [s[p + 1] - s[p] for p in range(len(names) - 1) if p in s and p + 1 in s]
                    nxt = stamps.get((k, role, blk + 1), {}).get(0)
                    whole = f"  block {nxt - s[0]}" if nxt else ""
                    if nxt and role == 1:
                        per_block.append(nxt - s[0])
                    print(f"    role {role} block {blk:2d}: " + " ".join(f"{x:6d}" for x in d) + whole)
            if per_block:
                print(f"    rounds wave, top to top: median {sorted(per_block)[len(per_block) // 2]} ticks per block")


if __name__ == "__main__":
    main()
