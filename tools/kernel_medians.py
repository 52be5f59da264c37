#!/usr/bin/env python
"""kernel_medians.py DIR [NAME-PART ...]: launches, median and minimum duration (us) per kernel of a rocprofv3 --kernel-trace run."""
import csv
import glob
import os
import statistics
import sys
from collections import defaultdict

d, want = sys.argv[1], sys.argv[2:]
per = defaultdict(list)
for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
    with open(f, newline="") as fh:
        for r in csv.DictReader(fh):
            per[r["Kernel_Name"].split("(")[0].replace("void ", "").replace("zke::", "")].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
for name, v in sorted(per.items(), key=lambda kv: -sum(kv[1])):
    if not want or any(w in name for w in want):
        print(f"{name[:48]:48s} launches {len(v):5d}  median {1e-3 * statistics.median(v):8.2f} us  min {1e-3 * min(v):8.2f} us")
