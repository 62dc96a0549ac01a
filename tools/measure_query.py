#!/usr/bin/env python3
"""Time kmc_query_device and kmc_profile_device on the views real finalizes leave.

Tables: synth pool 0 (every line fresh random: all-distinct, the sort path) and the benchmark's pool-10 generator input (a
few thousand keys), k = 31, --gb GB of FASTA each.  Per table:
  * index build: the first query of the view (one key), minus a warm query of one key; index bytes from the key count;
  * lookups/s for --queries random PRESENT keys (gathered from the view on the device) and as many ABSENT ones (random
    62-bit words; on the sparse tables here a random word is absent);
  * k-mers/s of a profile over the reads the table was counted from (window counts and read statistics);
  * beside the lookups, what the library offered before for the same answer: kmc_export to the host +
    numpy.searchsorted on the same keys (host clock), and a plain binary search over the whole view on the device
    (torch.searchsorted on the view's key array: a comparator of this tool only, not product code).
The ctx runs on a torch stream, so device times are event pairs on that stream around warm calls: --warmup untimed, --reps
timed, the median reported (and the minimum).  Bytes per lookup come from a separate `rocprofv3 --pmc` run of this tool.
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


def measure(args, pool, k=31):
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    rows = []
    with torch.cuda.stream(stream):
        s = kmc.Synth(seed=1, pool=pool)
        n_rec, _ = kmc.synth_records_for_bytes(s, int(args.gb * 1e9))
        n_bases = n_rec * s.read_len
        d_b = torch.empty(n_bases + 64, dtype=torch.uint8, device=dev)
        d_o = torch.empty(n_rec + 1, dtype=torch.int64, device=dev)
        kmc.synth_reads_device(s, 0, n_rec, d_b.data_ptr(), d_o.data_ptr(), 0, stream.cuda_stream)
        stream.synchronize()
        kc = kmc.KmerCounter(k=k, stream=stream.cuda_stream)
        kc.add_batch_device(d_b.data_ptr(), d_o.data_ptr(), n_rec, n_bases, s.read_len)
        nd, nt = kc.finalize()
        name = f"pool{pool}_k{k} ({args.gb:g} GB, {nd} keys)"
        _, p_lo, p_cnt, _ = kc.export_device()
        v_lo = kd.device_view(p_lo, nd, dev)
        v_cnt = kd.device_view(p_cnt, nd, dev)
        nq = args.queries
        g = torch.Generator(device=dev)
        g.manual_seed(5)
        present = v_lo[torch.randint(0, nd, (nq,), device=dev, generator=g)].contiguous()
        absent = torch.randint(0, 2**62, (nq,), device=dev, generator=g, dtype=torch.int64)
        out = torch.empty(nq, dtype=torch.int64, device=dev)
        one = present[:1].clone()
        stream.synchronize()
        # index build = first query of the view - a warm query
        t_first, _ = ev_timed(stream, lambda: kc.query_device(0, one.data_ptr(), 1, out.data_ptr()), 0, 1)
        t_warm, _ = ev_timed(stream, lambda: kc.query_device(0, one.data_ptr(), 1, out.data_ptr()), 2, 5)
        bits = min(27, 2 * k, max(0, int(nd).bit_length() - 1))
        rows.append(dict(table=name, call="index_build", ms=t_first - t_warm, index_bytes=4 * (2**bits + 1), index_bits=bits))
        for label, q in (("present", present), ("absent", absent)):
            med, mn = ev_timed(stream, lambda: kc.query_device(0, q.data_ptr(), nq, out.data_ptr()), args.warmup, args.reps)
            stream.synchronize()
            hits = int((out != 0).sum())
            # plain binary search over the whole view on the device (tool-only comparator)
            def plain():
                pos = torch.searchsorted(v_lo, q).clamp_(max=nd - 1)
                return torch.where(v_lo[pos] == q, v_cnt[pos], torch.zeros_like(q))
            pmed, pmn = ev_timed(stream, plain, args.warmup, args.reps)
            assert torch.equal(plain(), out)
            rows.append(dict(table=name, call="kmc_query_device", keys=label, n=nq, hits=hits, ms_median=med, ms_min=mn,
                             lookups_per_s=nq / (med * 1e-3), plain_search_ms_median=pmed, ratio_plain_over_indexed=pmed / med))
        # what the library offered before: export to the host + numpy.searchsorted
        qh = present.cpu().numpy().view(np.uint64)
        t0 = time.perf_counter()
        t = kc.export()
        t1 = time.perf_counter()
        pos = np.minimum(np.searchsorted(t.key_lo, qh), nd - 1)
        ans = np.where(t.key_lo[pos] == qh, t.count[pos], 0)
        t2 = time.perf_counter()
        kc.query_device(0, present.data_ptr(), nq, out.data_ptr())
        stream.synchronize()
        assert np.array_equal(ans.astype(np.uint64), out.cpu().numpy().view(np.uint64))
        rows.append(dict(table=name, call="export+numpy.searchsorted", keys="present", n=nq, export_ms=(t1 - t0) * 1e3,
                         search_ms=(t2 - t1) * 1e3))
        del t
        # profile of the counted reads themselves
        win = torch.empty(n_bases, dtype=torch.int32, device=dev)
        rs = torch.empty((n_rec, 5), dtype=torch.int64, device=dev)
        for label, w, r in (("windows+stats", win, rs), ("windows", win, None), ("stats", None, rs)):
            f = lambda: kc.profile_device(d_b.data_ptr(), d_o.data_ptr(), n_rec, n_bases, 1, w.data_ptr() if w is not None else 0,
                                          r.data_ptr() if r is not None else 0)
            med, mn = ev_timed(stream, f, args.warmup, args.reps)
            n_win = n_rec * (s.read_len - k + 1)
            rows.append(dict(table=name, call="kmc_profile_device", outputs=label, bases=n_bases, windows=n_win, ms_median=med, ms_min=mn,
                             kmers_per_s=n_win / (med * 1e-3)))
        stream.synchronize()
        assert int(rs[:, 4].sum()) >= nt and int(rs[:, 0].sum()) == n_win
        kc.close()
    del d_b, d_o
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=1.0)
    ap.add_argument("--queries", type=int, default=1 << 24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--pools", default="0,10")
    ap.add_argument("--small", action="store_true", help="a quick pass: 0.05 GB, 2^20 queries")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.small:
        args.gb, args.queries = 0.05, 1 << 20
    rows = []
    for pool in [int(x) for x in args.pools.split(",")]:
        for r in measure(args, pool):
            print(json.dumps(r), flush=True)
            rows.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
