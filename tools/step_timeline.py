#!/usr/bin/env python3
"""One benchmark step out of a rocprofv3 kernel trace (tools/profile_bench.sh): every kernel from the start of a walk
kernel to the start of the next one, as start / gap / duration in microseconds -- the format of profiles/r0*_step_timeline.txt.
usage: tools/step_timeline.py <kernel_trace.csv> [step]      (step: which walk kernel from the END opens the table, default 3)"""
import csv
import sys


def main():
    path = sys.argv[1]
    back = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].split("(")[0]))
    rows.sort()
    walks = [i for i, r in enumerate(rows) if "kmc_walk_kernel" in r[2]]
    if len(walks) < back:
        raise SystemExit("fewer than %d walk kernels in %s" % (back, path))
    a, b = walks[-back], walks[-back + 1] if back > 1 else len(rows) - 1
    t0 = rows[a][0]
    print("   start us    gap us     dur us  kernel")
    prev_end = t0
    for s, e, name in rows[a:b + 1]:
        print("%10.1f %9.1f %10.1f  %s" % ((s - t0) / 1e3, (s - prev_end) / 1e3, (e - s) / 1e3, name))
        prev_end = e


if __name__ == "__main__":
    main()
