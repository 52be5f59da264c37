#!/usr/bin/env python
"""sha_twin_timeline.py [--reps K] [--timeout S] [--reports PLAIN STAMPED]: sha256_ring_kernel against sha256_twin_kernel alone, and what a block costs their waves.

Builds tests/cpp/sha_twin_probe twice (build.build_sha_twin_probe: without stamps, the code the library runs, and with
ZKE_SHA_PROBE) and runs each ONCE, under a time limit, on 1 024 messages of 4 KB (65 blocks).  Prints
  * from the plain build: each kernel's median time over K launches, per block, and whether its digests are hashlib's;
  * from the stamped build, for blocks 8..15 of group 0 and per wave: ticks of work and ticks at the barrier.  The ring stamps
    every block in both waves; the twin's rounds wave stamps every block (a barrier behind the odd ones), its feeder every pass
    of two blocks.
--reports prints from two reports that the probe wrote earlier (sha_twin_probe_plain, sha_twin_probe) instead of running it.
profiles/sha_twin_timeline.txt is this program's output."""
import argparse
import collections
import hashlib
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEN, BLOCKS = 4096, 65


def message(i):
    return bytes((131 * i + 7 * j + (j >> 8)) & 255 for j in range(LEN))


def run(exe, reps, timeout):
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "report.txt")
        r = subprocess.run([exe, path, str(reps)], timeout=timeout, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            raise SystemExit("sha_twin_probe exited with %d" % r.returncode)
        return [ln.split() for ln in open(path)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--timeout", type=int, default=120)
    ap.add_argument("--reports", nargs=2, metavar=("PLAIN", "STAMPED"))
    args = ap.parse_args()
    if args.reports:
        plain, lines = ([ln.split() for ln in open(f)] for f in args.reports)
    else:
        from zkemail_rs_amd import build
        plain = run(build.build_sha_twin_probe(stamps=False), args.reps, args.timeout)
        lines = run(build.build_sha_twin_probe(stamps=True), args.reps, args.timeout)
    print("build without stamps")
    for ln in plain:
        if ln[0] == "time":
            print(f"{ln[1]}: median {float(ln[2]):.1f} us, best {float(ln[3]):.1f} us over {args.reps} launches; {float(ln[2]) / BLOCKS:.3f} us per block")
    for ln in plain:
        if ln[0] == "digest":
            ok = hashlib.sha256(message(int(ln[2]))).hexdigest() == ln[3]
            print(f"digest {ln[1]} message {ln[2]}: {'hashlib' if ok else 'WRONG'}")
            if not ok:
                raise SystemExit(1)
    print()
    print("build with stamps (ZKE_SHA_PROBE): the stamps cost time themselves")
    for ln in lines:
        if ln[0] == "time":
            print(f"{ln[1]}: median {float(ln[2]):.1f} us; {float(ln[2]) / BLOCKS:.3f} us per block")
    stamps = collections.defaultdict(dict)
    for ln in lines:
        if ln[0] == "stamp":
            stamps[(ln[1], int(ln[2]), int(ln[3]))][int(ln[4])] = int(ln[5])
    print("group 0, blocks 8..15, clock ticks: loop top -> work done -> after the barrier (role 0 feeder, 1 rounds)")
    for k in ("ring", "twin"):
        for role in (0, 1):
            step = 2 if (k == "twin" and role == 0) else 1
            tops = []
            for blk in range(8, 16, step):
                s = stamps.get((k, role, blk))
                if not s or 0 not in s or 1 not in s or 2 not in s:
                    continue
                nxt = stamps.get((k, role, blk + step), {}).get(0)
                if nxt:
                    tops.append(nxt - s[0])
                unit = "pass of two blocks" if step == 2 else "block"
                print(f"  {k} role {role} block {blk:2d}: work {s[1] - s[0]:6d}  barrier {s[2] - s[1]:6d}" + (f"  {unit} {nxt - s[0]}" if nxt else ""))
            if tops:
                print(f"  {k} role {role}: median {sorted(tops)[len(tops) // 2] // step} ticks per block, top to top")


if __name__ == "__main__":
    main()
