#!/usr/bin/env python3
"""Time kmc_histogram and kmc_filter_device on the views real finalizes leave.

Tables: synth pool 0 (every line fresh random: the sort path, every count 1) at --gb GB of FASTA for k=31 and k=63; the
benchmark's pool-10 generator input at the same size; a kmc_merge_pairs_device table of --pairs keys with counts drawn
from a spectrum-like law.  Per table: the finalize time (host clock around the synchronous call), then per call
--warmup untimed calls and --reps timed ones (host clock around each call: both calls synchronise before they return).
Bytes model: the histogram reads 8 B per key; the filter reads 8*KW + 8 B per key plus the counts a second time, and
writes 8*KW + 8 B per kept key.  Fractions are of the nominal 8 TB/s.  Kernel times come from a separate
`rocprofv3 --kernel-trace --stats` run of this tool (--reps 3).  One JSON line per measurement on stdout; --out also
writes them all to a file."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

kmc = importlib.import_module("k-mer-count_amd")
HBM = 8e12


def timed(f, warmup, reps):
    for _ in range(warmup):
        f()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return min(ts), float(np.median(ts))


def spectrum_rows(kc, name, kw, fin_s, args):
    nd = kc.export_device()[3]
    rows = []
    t_min, t_med = timed(lambda: kc.histogram(10001), args.warmup, args.reps)
    b = 8.0 * nd
    rows.append(dict(table=name, call="kmc_histogram", n_bins=10001, keys=nd, ms_min=t_min * 1e3, ms_median=t_med * 1e3,
                     bytes=b, frac_8TBs=b / t_min / HBM, finalize_ms=fin_s * 1e3))
    h = kc.histogram(10001)
    # two filters: min 2 (drops the singletons: the common error cutoff) and [1, 1] (keeps the singletons)
    for lo, hi in ((2, 0), (1, 1)):
        nk = kc.filter_device(lo, hi)[3]
        t_min, t_med = timed(lambda: kc.filter_device(lo, hi), args.warmup, args.reps)
        b = (8.0 * kw + 16.0) * nd + (8.0 * kw + 8.0) * nk
        rows.append(dict(table=name, call="kmc_filter_device", min_count=lo, max_count=hi, keys=nd, kept=nk,
                         ms_min=t_min * 1e3, ms_median=t_med * 1e3, bytes=b, frac_8TBs=b / t_min / HBM, finalize_ms=fin_s * 1e3))
    rows.append(dict(table=name, call="spectrum_head", hist_1_to_8=[int(x) for x in h[1:9]], distinct=nd))
    return rows


def synth_table(args, k, pool):
    s = kmc.Synth(seed=1, pool=pool)
    n_rec, _ = kmc.synth_records_for_bytes(s, int(args.gb * 1e9))
    d_b = torch.empty(n_rec * s.read_len + 64, dtype=torch.uint8, device="cuda")
    d_o = torch.empty(n_rec + 1, dtype=torch.int64, device="cuda")
    kmc.synth_reads_device(s, 0, n_rec, d_b.data_ptr(), d_o.data_ptr())
    torch.cuda.synchronize()
    kc = kmc.KmerCounter(k=k)
    step = (n_rec + 3) // 4
    for first in range(0, n_rec, step):   # four batches, like the file pipeline's chunks
        n = min(step, n_rec - first)
        d_o2 = (d_o[first:first + n + 1] - d_o[first]).contiguous()
        kc.add_batch_device(d_b.data_ptr() + first * s.read_len, d_o2.data_ptr(), n, n * s.read_len, s.read_len)
    kc.poll()
    t0 = time.perf_counter()
    kc.finalize()
    fin = time.perf_counter() - t0
    del d_b, d_o
    torch.cuda.empty_cache()
    return kc, fin


def pairs_table(args, k):
    rng = np.random.default_rng(7)
    n = args.pairs
    lo = np.unique(rng.integers(0, 2**62, n + n // 8, dtype=np.uint64))[:n]
    n = lo.size
    hi = rng.integers(0, 2**60, n, dtype=np.uint64) if k > 31 else np.zeros(n, np.uint64)
    cnt = np.minimum(rng.zipf(1.6, n), 1 << 20).astype(np.uint64)   # most keys at 1..3, a long tail
    perm = rng.permutation(n)
    dev = lambda a: torch.from_numpy(a[perm].astype(np.int64)).cuda()
    d_lo, d_hi, d_c = dev(lo), dev(hi), dev(cnt)
    kc = kmc.KmerCounter(k=k)
    kc.merge_pairs_device(d_hi.data_ptr() if k > 31 else 0, d_lo.data_ptr(), d_c.data_ptr(), n)
    kc.poll()
    t0 = time.perf_counter()
    kc.finalize()
    fin = time.perf_counter() - t0
    return kc, fin


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=1.0)
    ap.add_argument("--pairs", type=int, default=100_000_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cases", default="pool0_k31,pool0_k63,pool10_k31,pairs_k31")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rows = []
    for case in args.cases.split(","):
        if case.startswith("pairs"):
            k = int(case.split("_k")[1])
            kc, fin = pairs_table(args, k)
        else:
            pool = int(case.split("_")[0][4:])
            k = int(case.split("_k")[1])
            kc, fin = synth_table(args, k, pool)
        name = f"{case} ({args.gb:g} GB)" if not case.startswith("pairs") else f"{case} ({args.pairs} pairs)"
        for r in spectrum_rows(kc, name, 1 if k <= 31 else 2, fin, args):
            print(json.dumps(r), flush=True)
            rows.append(r)
        kc.close()
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
