#!/usr/bin/env python3
"""Time kmc_compare and kmc_setop_device on pairs of views real finalizes leave.

Pairs, k = 31: two half-overlapping ranges of synth pool 0 records (all-distinct input, the sort path; --gb GB of FASTA each:
records [0, n) against [n/2, 3n/2)), and the same ranges of the benchmark's pool-10 generator input (a few thousand keys).
Per pair: kmc_compare, kmc_setop_device INTERSECT+MIN, UNION+SUM, SUBTRACT+LEFT.  Both contexts run on one torch stream, so
device times are event pairs on that stream around warm calls (--warmup untimed, --reps timed; median and minimum).  The
calls wait for their result, so an event pair spans the whole call.  Algorithmic bytes: compare reads 16 (n_a + n_b) for
one-word keys; a set operation reads that twice (count pass, scatter pass) and writes 16 n_out; the fraction is of 8 TB/s.
Beside them, for the intersection's counts, what the parent offered: (a) export of both tables + numpy join on the host,
(b) kmc_query_device of A's keys against B (counts only, no ordered union).
--skew N: crafted views of N keys through kmc_merge_pairs_device -- strictly interleaved, A below B, B below A, one key
against N -- timed per merged key; merge-path tiles must make them run at the same rate.
Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this tool.
One JSON line per measurement on stdout; --out also writes them all to a file."""
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
kd = importlib.import_module("k-mer-count_amd.distributed")
HBM_PEAK = 8e12
CASES = (("intersect", "min"), ("union", "sum"), ("subtract", "left"))


def ev_timed(stream, f, warmup, reps):
    for _ in range(warmup):
        f()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        f()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms))


def time_pair(args, stream, name, ka, kb, rows, kw=1):
    ent = 8 * kw + 8
    c = ka.compare(kb)
    n_in = c.n_a + c.n_b
    med, mn = ev_timed(stream, lambda: ka.compare(kb), args.warmup, args.reps)
    rows.append(dict(pair=name, call="kmc_compare", n_a=c.n_a, n_b=c.n_b, n_both=c.n_both, jaccard=c.jaccard, ms_median=med, ms_min=mn,
                     bytes=ent * n_in, frac_hbm_peak=ent * n_in / (med * 1e-3) / HBM_PEAK, ns_per_key=med * 1e6 / max(n_in, 1)))
    for op, mode in CASES:
        n_out = ka.setop_device(kb, op, mode)[3]
        med, mn = ev_timed(stream, lambda: ka.setop_device(kb, op, mode), args.warmup, args.reps)
        by = 2 * ent * n_in + ent * n_out
        rows.append(dict(pair=name, call="kmc_setop_device", op=op, counts=mode, n_out=n_out, ms_median=med, ms_min=mn, bytes=by,
                         frac_hbm_peak=by / (med * 1e-3) / HBM_PEAK, ns_per_key=med * 1e6 / max(n_in, 1)))
    return c


def measure_counted(args, pool, k=31):
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    rows = []
    with torch.cuda.stream(stream):
        s = kmc.Synth(seed=1, pool=pool)
        n_rec, _ = kmc.synth_records_for_bytes(s, int(args.gb * 1e9))
        ctxs = []
        for first in (0, n_rec // 2):
            n_bases = n_rec * s.read_len
            d_b = torch.empty(n_bases + 64, dtype=torch.uint8, device=dev)
            d_o = torch.empty(n_rec + 1, dtype=torch.int64, device=dev)
            kmc.synth_reads_device(s, first, n_rec, d_b.data_ptr(), d_o.data_ptr(), 0, stream.cuda_stream)
            stream.synchronize()
            kc = kmc.KmerCounter(k=k, stream=stream.cuda_stream)
            kc.add_batch_device(d_b.data_ptr(), d_o.data_ptr(), n_rec, n_bases, s.read_len)
            kc.finalize()
            ctxs.append(kc)
            del d_b, d_o
        ka, kb = ctxs
        name = f"pool{pool}_k{k} ({args.gb:g} GB each, half overlap)"
        c = time_pair(args, stream, name, ka, kb, rows)
        # (b) the parent's device route to the intersection's counts: A's keys looked up in B
        _, a_lo, _, na = ka.export_device()
        out = torch.empty(max(na, 1), dtype=torch.int64, device=dev)
        med, mn = ev_timed(stream, lambda: kb.query_device(0, a_lo, na, out.data_ptr()), args.warmup, args.reps)
        stream.synchronize()
        assert int((out[:na] != 0).sum()) == c.n_both
        rows.append(dict(pair=name, call="kmc_query_device(A keys in B)", n=na, ms_median=med, ms_min=mn))
        # (a) the parent's host route: export both, join in numpy
        t0 = time.perf_counter()
        ta, tb = ka.export(), kb.export()
        t1 = time.perf_counter()
        _, ia, ib = np.intersect1d(ta.key_lo, tb.key_lo, assume_unique=True, return_indices=True)
        m = np.minimum(ta.count[ia], tb.count[ib])
        t2 = time.perf_counter()
        assert ia.shape[0] == c.n_both and int(m.sum(dtype=np.uint64)) == c.sum_min
        rows.append(dict(pair=name, call="export both + numpy.intersect1d", export_ms=(t1 - t0) * 1e3, join_ms=(t2 - t1) * 1e3))
        del ta, tb
        ka.close()
        kb.close()
    torch.cuda.empty_cache()
    return rows


def crafted(stream, dev, vals):
    kc = kmc.KmerCounter(k=31, stream=stream.cuda_stream)
    cnt = torch.ones_like(vals)
    kc.merge_pairs_device(0, vals.data_ptr(), cnt.data_ptr(), vals.numel())
    kc.finalize()
    stream.synchronize()
    return kc


def measure_skew(args):
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    rows = []
    n = args.skew
    with torch.cuda.stream(stream):
        ar = torch.arange(n, dtype=torch.int64, device=dev)
        shapes = (("interleaved", 2 * ar, 2 * ar + 1), ("a_below_b", ar, ar + 4 * n), ("b_below_a", ar + 4 * n, ar),
                  ("one_vs_n", torch.tensor([n], dtype=torch.int64, device=dev), 2 * ar), ("identical", 3 * ar, 3 * ar))
        for label, va, vb in shapes:
            ka, kb = crafted(stream, dev, va), crafted(stream, dev, vb)
            time_pair(args, stream, f"skew_{label} ({n} keys)", ka, kb, rows)
            ka.close()
            kb.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--pools", default="0,10")
    ap.add_argument("--skew", type=int, default=1 << 24, help="keys per crafted view of the skew check (0: skip)")
    ap.add_argument("--small", action="store_true", help="a quick pass: 0.05 GB, 2^20-key skew views")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.small:
        args.gb, args.skew = 0.05, 1 << 20
    rows = []
    for pool in [int(x) for x in args.pools.split(",") if x]:
        for r in measure_counted(args, pool):
            print(json.dumps(r), flush=True)
            rows.append(r)
    if args.skew:
        for r in measure_skew(args):
            print(json.dumps(r), flush=True)
            rows.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
