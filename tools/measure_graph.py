#!/usr/bin/env python3
"""Time kmc_graph_device on the views real finalizes leave, beside the same answer obtained with what the
library offered before it.

Tables: synth pool 0 (every line fresh random: all-distinct, the sort path) and the benchmark's pool-10 generator input (a
few thousand keys), k = 31, --gb GB of FASTA each, canonical and forward.  Per table:
  * index build: the first query of the view (one key), minus a warm query of one key;
  * kmc_graph_device for the ranges (1, 0) and (2, 0): median and minimum, and lookups/s = 14 n / time (8 neighbour and 6
    sibling keys per view key; the kernel skips the lookups of keys that are not solid, the figure does not);
  * the comparator, a thing of this tool only and not product code: the 14 n neighbour and sibling keys built from the view
    with torch operations on the device (shifts, masks, a log-step reverse complement, minimum for the canonical strand),
    resolved with kmc_query_device, folded into adj words and the summary with torch again -- in chunks of --chunk view keys,
    as a user short of 14 x 8 n bytes would.  Its key-building time counts: a user pays it.  Its result must equal the
    kernel's, word for word;
  * the comparator's kmc_query_device calls alone (lookups/s of the query kernel on these keys).
The ctx runs on a torch stream, so device times are event pairs on that stream: --warmup untimed, --reps timed, the median
reported (and the minimum).  One JSON line per measurement on stdout; --out also writes them all to a file."""
import argparse
import importlib
import json
import os
import sys

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


def revcomp62(x, k):
    """reverse complement of one-word keys (int64 tensor, 2k <= 62 bits): complement, reverse the 32 base pairs, shift down"""
    y = ~x
    for s, m in ((2, 0x3333333333333333), (4, 0x0F0F0F0F0F0F0F0F), (8, 0x00FF00FF00FF00FF), (16, 0x0000FFFF0000FFFF),
                 (32, 0x00000000FFFFFFFF)):
        y = ((y >> s) & m) | ((y & m) << s)
    return (y >> (64 - 2 * k)) & ((1 << (2 * k)) - 1)


class Comparator:
    """adj and summary of the view from 14 n kmc_query_device lookups on keys built with torch."""

    def __init__(self, kc, k, canonical, v_lo, v_cnt, chunk):
        self.kc, self.k, self.canonical, self.v_lo, self.v_cnt, self.chunk = kc, k, canonical, v_lo, v_cnt, chunk
        self.n = v_lo.numel()
        self.adj = torch.empty(self.n, dtype=torch.int16, device=v_lo.device)
        m = min(chunk, max(self.n, 1))
        self.keys = torch.empty((14, m), dtype=torch.int64, device=v_lo.device)
        self.cnt = torch.empty((14, m), dtype=torch.int64, device=v_lo.device)
        self.query_ms = 0.0

    def build(self, x):
        k, tb, mask = self.k, 2 * self.k - 2, (1 << (2 * self.k)) - 1
        top = 3 << tb
        m = x.numel()
        K = self.keys[:, :m]
        r = revcomp62(x, k) if self.canonical else None
        xs, xr = (x << 2) & mask, x >> 2
        x_top0, x_low0 = x & ~top, x & ~3
        if r is not None:
            rs, rr = (r << 2) & mask, r >> 2
            r_top0, r_low0 = r & ~top, r & ~3
        first, last = x >> tb, x & 3
        row = 8
        for c in range(4):
            f, g = xs | c, xr | (c << tb)
            if r is not None:
                f = torch.minimum(f, rr | ((3 - c) << tb))
                g = torch.minimum(g, rs | (3 - c))
            K[c], K[4 + c] = f, g
        # the three siblings on either side that are not x itself: d = (own base + 1, 2, 3) mod 4
        for j in (1, 2, 3):
            d = (first + j) & 3
            f = x_top0 | (d << tb)
            e = (last + j) & 3
            g = x_low0 | e
            if r is not None:
                f = torch.minimum(f, r_low0 | (3 - d))
                g = torch.minimum(g, r_top0 | ((3 - e) << tb))
            K[row], K[row + 3] = f, g
            row += 1
        return K

    def run(self, lo_c, hi_c, timed_query=False):
        hi_c = hi_c or (1 << 62)
        words = torch.zeros(8, dtype=torch.int64, device=self.v_lo.device)
        for a in range(0, self.n, self.chunk):
            x, xc = self.v_lo[a:a + self.chunk], self.v_cnt[a:a + self.chunk]
            m = x.numel()
            K = self.build(x).contiguous()
            C = self.cnt[:, :m].contiguous()
            if timed_query:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(torch.cuda.current_stream())
            self.kc.query_device(0, K.data_ptr(), 14 * m, C.data_ptr())
            if timed_query:
                e1.record(torch.cuda.current_stream())
                e1.synchronize()
                self.query_ms += e0.elapsed_time(e1)
            S = (C >= lo_c) & (C <= hi_c)
            solid = (xc >= lo_c) & (xc <= hi_c)
            Si = S.to(torch.int64)
            dr, dl = Si[0:4].sum(0), Si[4:8].sum(0)
            # x itself is the fourth sibling on both sides (the view of a counting ctx holds keys of its own strand rule only)
            cont_r = (dr == 1) & (Si[8:11].sum(0) == 0)
            cont_l = (dl == 1) & (Si[11:14].sum(0) == 0)
            nb = sum(Si[u] << u for u in range(8))
            er, el = (~cont_r).to(torch.int64), (~cont_l).to(torch.int64)
            adj = torch.where(solid, nb | (er << 8) | (el << 9) | 1024, torch.zeros_like(nb))
            self.adj[a:a + m] = adj.to(torch.int16)
            so = solid.to(torch.int64)
            words += torch.stack([so.sum(), (dr * so).sum(), (dl * so).sum(), (so * ((dr == 0) & (dl == 0))).sum(),
                                  (so * ((dr == 0) != (dl == 0))).sum(), (so * ((dr >= 2) | (dl >= 2))).sum(),
                                  (so * (er + el)).sum(), (so * er * el).sum()])
        return words


def measure(args, pool, canonical, k=31):
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
        kc = kmc.KmerCounter(k=k, canonical=canonical, stream=stream.cuda_stream)
        kc.add_batch_device(d_b.data_ptr(), d_o.data_ptr(), n_rec, n_bases, s.read_len)
        nd, nt = kc.finalize()
        del d_b, d_o
        torch.cuda.empty_cache()
        name = f"pool{pool}_k{k}_{'canonical' if canonical else 'forward'} ({args.gb:g} GB, {nd} keys)"
        _, p_lo, p_cnt, _ = kc.export_device()
        v_lo, v_cnt = kd.device_view(p_lo, nd, dev), kd.device_view(p_cnt, nd, dev)
        one = v_lo[:1].clone()
        out1 = torch.empty(1, dtype=torch.int64, device=dev)
        stream.synchronize()
        t_first, _ = ev_timed(stream, lambda: kc.query_device(0, one.data_ptr(), 1, out1.data_ptr()), 0, 1)
        t_warm, _ = ev_timed(stream, lambda: kc.query_device(0, one.data_ptr(), 1, out1.data_ptr()), 2, 5)
        rows.append(dict(table=name, call="index_build", ms=t_first - t_warm))
        comp = Comparator(kc, k, canonical, v_lo, v_cnt, args.chunk)
        for lo_c, hi_c in ((1, 0), (2, 0)):
            res = {}
            med, mn = ev_timed(stream, lambda: res.update(g=kc.graph_device(lo_c, hi_c)), args.warmup, args.reps)
            ptr, n, summ = res["g"]
            cmed, cmn = ev_timed(stream, lambda: res.update(w=comp.run(lo_c, hi_c)), args.warmup, args.reps)
            comp.query_ms = 0.0
            comp.run(lo_c, hi_c, timed_query=True)
            stream.synchronize()
            got = kd.device_view(ptr, (2 * n + 7) // 8, dev).view(torch.int16)[:n]
            same = bool(torch.equal(got, comp.adj)) and res["w"].tolist() == summ.words()
            rows.append(dict(table=name, call="kmc_graph_device", range=[lo_c, hi_c], n=nd, summary=summ.words(), ms_median=med, ms_min=mn,
                             lookups_per_s=14 * nd / (med * 1e-3), comparator_ms_median=cmed, comparator_ms_min=cmn,
                             ratio_comparator_over_graph=cmed / med, comparator_query_only_ms=comp.query_ms,
                             query_lookups_per_s=14 * nd / (comp.query_ms * 1e-3), comparator_equal=same))
            assert same, "the comparator and kmc_graph_device disagree"
        kc.close()
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--pools", default="0,10")
    ap.add_argument("--chunk", type=int, default=1 << 25, help="view keys per comparator pass")
    ap.add_argument("--small", action="store_true", help="a quick pass: 0.05 GB")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.small:
        args.gb = 0.05
    rows = []
    for pool in [int(x) for x in args.pools.split(",")]:
        for canonical in (True, False):
            for r in measure(args, pool, canonical):
                print(json.dumps(r), flush=True)
                rows.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
