#!/usr/bin/env python3
"""Time the clean pass of kmc_unitig_clean_device, one full cleaning round, and the same answer on the host.

Tables, k = 31, canonical and forward: the benchmark's pool-10 generator input (a few thousand keys, --gb GB of FASTA) and
synth pool 0 (every line fresh random: all-distinct, --gb-distinct GB; 0.05 GB gives the 41.9 M-key tables of §4.11 / §4.12).
Per table, in a child process with KMC_UNITIG_TRACE set so that the library prints its own event times:
  * one kmc_unitig_links_device call, then --reps kmc_unitig_clean_device calls behind it, which find the unitigs and the
    links in the ctx and run the clean pass alone: clean_ms, median and minimum, and the same calls timed from outside;
  * --reps full rounds: kmc_unitig_clean_into a fresh ctx and kmc_finalize of it, wall time (the unitigs and links of the
    source are held, so a round is clean + merge + finalize);
  * the read peak of the device as bench.py takes it (kmc_read_peak_device, the best of its four grid shapes, over 2 GiB)
    beside the bytes the pass must move (the view's keys and counts once, the kept entries written) and a lower-bound model
    of what it does move (adj and the ranking of every row on top); fractions of the nominal 8 TB/s, as §4.7 quotes them,
    and of the measured peak;
  * host_clean: the same verdicts and kept table with numpy from kmc_unitigs + kmc_unitig_links + kmc_export, timed, and
    compared with the device's.
One JSON line per table on stdout; --out also writes them to a file.
clean_ms spans the whole pass, host round trips between its launches included.  The split by launch comes from a kernel
trace of one child: rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/measure_clean.py --child
POOL,CANONICAL,K,TIP,ISLAND --gb GB --no-host, then --split-from-trace DIR/.../*_kernel_trace.csv."""
import argparse
import importlib
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

U64 = np.uint64
UNLIMITED = 1 << 31
NOMINAL_GBS = 8000.0   # the HBM peak §4.7 quotes its fractions against


def _mul128(a, b):
    """(high, low) words of the products of two uint64 arrays"""
    m = U64(0xFFFFFFFF)
    s = U64(32)
    a0, a1, b0, b1 = a & m, a >> s, b & m, b >> s
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = (p00 >> s) + (p01 & m) + (p10 & m)
    return p11 + (p01 >> s) + (p10 >> s) + (mid >> s), (p00 & m) | (mid << s)


def host_verdicts(offsets, abund, flags, link_offsets, link_to, k, max_tip, max_island):
    """The verdict per unitig (include/kmc.h) from the arrays of kmc_unitigs and kmc_unitig_links, vectorised"""
    nu = len(abund)
    if not nu:
        return np.zeros(0, np.uint8)
    m = (np.diff(offsets) - U64(k - 1)).astype(U64)
    lo = link_offsets.astype(np.int64)
    r0, r1 = lo[1:2 * nu:2] - lo[0:2 * nu:2], lo[2:2 * nu + 1:2] - lo[1:2 * nu:2]
    circ = (flags & 1) != 0
    fits = lambda lim: np.ones(nu, bool) if lim >= UNLIMITED else m <= U64(lim)
    island = ~circ & (r0 == 0) & (r1 == 0) & fits(max_island)
    cand = ~circ & fits(max_tip) & (((r0 == 0) & (r1 == 1)) | ((r0 == 1) & (r1 == 0)))
    verdict = np.where(island, 2, 0).astype(np.uint8)
    u = np.flatnonzero(cand)
    if len(u):
        a = 2 * u + (r1[u] == 1)
        t = link_to[lo[a]].astype(np.int64)
        dominated = np.zeros(len(u), bool)
        for j in range(4):
            idx = lo[t] + j
            ok = idx < lo[t + 1]
            s = link_to[np.where(ok, idx, 0)].astype(np.int64)
            w = s >> 1
            ok &= (s != a) & (w != u)
            lh, ll = _mul128(abund[w], m[u])
            rh, rl = _mul128(abund[u], m[w])
            more = (lh > rh) | ((lh == rh) & (ll > rl))
            same = (lh == rh) & (ll == rl)
            beats = more | (same & ((m[w] > m[u]) | ((m[w] == m[u]) & (w < u))))
            dominated |= ok & (~cand[w] | beats)
        verdict[u[dominated]] = 1
    return verdict


def host_clean(table, unitigs, links, k, canonical, max_tip, max_island):
    """(key_lo, count, verdict, summary words) of the cleaned table from Table / Unitigs / UnitigLinks objects, k <= 31: the
    k-mers of the unitigs are spelled again with numpy, put in the ctx's key form and looked up in the table"""
    assert k <= 31
    verdict = host_verdicts(unitigs.offsets, unitigs.abund, unitigs.flags, links.offsets, links.to, k, max_tip, max_island)
    nu = len(verdict)
    words = [nu, int((verdict == 1).sum()), int((verdict == 2).sum()), 0, 0, 0, 0, 0]
    if not nu:
        return np.zeros(0, U64), np.zeros(0, U64), verdict, words
    code = np.zeros(256, U64)
    code[[ord(c) for c in "ACGT"]] = np.arange(4, dtype=U64)
    c = code[unitigs.bases]
    nb = len(c)
    fwd, rev = np.zeros(nb - k + 1, U64), np.zeros(nb - k + 1, U64)
    for j in range(k):
        x = c[j:nb - k + 1 + j]
        fwd |= x << U64(2 * (k - 1 - j))
        rev |= (U64(3) - x) << U64(2 * j)
    key = np.minimum(fwd, rev) if canonical else fwd
    offs = unitigs.offsets.astype(np.int64)
    m = np.diff(offs) - (k - 1)
    start = np.repeat(offs[:-1], m) + (np.arange(int(m.sum())) - np.repeat(np.cumsum(m) - m, m))
    v_of_key = np.repeat(verdict, m)
    kept = np.sort(key[start[v_of_key == 0]])
    row = np.searchsorted(table.key_lo, kept)
    assert np.array_equal(table.key_lo[row], kept)
    cnt = table.count[row]
    r0 = np.diff(links.offsets.astype(np.int64))
    fits = m <= max_tip if max_tip < UNLIMITED else np.ones(nu, bool)
    cand = ((unitigs.flags & 1) == 0) & fits & (((r0[0::2] == 0) & (r0[1::2] == 1)) | ((r0[0::2] == 1) & (r0[1::2] == 0)))
    words[3:] = [len(kept), int(m[verdict == 1].sum()), int(m[verdict == 2].sum()), int(cand.sum()), int(cnt.sum(dtype=U64))]
    return kept, cnt, verdict, words


def make_ctx(kmc, torch, gb, pool, canonical, k, stream, dev):
    s = kmc.Synth(seed=1, pool=pool)
    n_rec, _ = kmc.synth_records_for_bytes(s, int(gb * 1e9))
    n_bases = n_rec * s.read_len
    d_b = torch.empty(n_bases + 64, dtype=torch.uint8, device=dev)
    d_o = torch.empty(n_rec + 1, dtype=torch.int64, device=dev)
    kmc.synth_reads_device(s, 0, n_rec, d_b.data_ptr(), d_o.data_ptr(), 0, stream.cuda_stream)
    stream.synchronize()
    kc = kmc.KmerCounter(k=k, canonical=canonical, stream=stream.cuda_stream)
    kc.add_batch_device(d_b.data_ptr(), d_o.data_ptr(), n_rec, n_bases, s.read_len)
    nd, _ = kc.finalize()
    del d_b, d_o
    torch.cuda.empty_cache()
    return kc, nd


def child(spec, gb, reps, host):
    """one table: the calls whose trace lines the parent reads; everything else on stdout"""
    import torch
    kmc = importlib.import_module("k-mer-count_amd")
    kd = importlib.import_module("k-mer-count_amd.distributed")
    pool, canonical, k, tip, isl = [int(x) for x in spec.split(",")]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    out = {}

    def ev_ms(f):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        f()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    with torch.cuda.stream(stream):
        kc, nd = make_ctx(kmc, torch, gb, pool, bool(canonical), k, stream, dev)
        kc.unitig_links_device(1, 0)
        kc.clean_unitigs_device(1, 0, tip, isl)          # warm: the buffers exist
        print("mark clean", file=sys.stderr, flush=True)
        res = {}
        ms = [ev_ms(lambda: res.update(r=kc.clean_unitigs_device(1, 0, tip, isl))) for _ in range(reps)]
        dh, dl, dc, dv, nk, nu, summ = res["r"]
        out.update(keys=nd, summary=summ.words(), call_ms_median=float(np.median(ms)), call_ms_min=float(min(ms)))
        print("mark rounds", file=sys.stderr, flush=True)
        wall = []
        for _ in range(reps):
            dst = kmc.KmerCounter(k=k, canonical=bool(canonical))
            t0 = time.perf_counter()
            kc.clean_into(dst, 1, 0, tip, isl)
            n_dst = dst.finalize()[0]
            wall.append((time.perf_counter() - t0) * 1e3)
            dst.close()
        out.update(round_ms_median=float(np.median(wall)), round_ms_min=float(min(wall)), round_keys=n_dst)
        print("mark end", file=sys.stderr, flush=True)
        # the streaming-read peak as bench.py takes it: the best of the four grid shapes, here over a buffer of 2 GiB
        if nd >= 1 << 20:
            buf = torch.zeros(1 << 31, dtype=torch.uint8, device=dev)
            stream.synchronize()
            best = max((buf.numel() / kmc.read_peak_device(buf.data_ptr(), buf.numel(), 0, stream.cuda_stream, shape, 5)[0] / 1e6, shape)
                       for shape in range(4))
            out["read_peak_gbs"], out["read_peak_shape"] = best
            del buf
        else:
            out["read_peak_gbs"] = None
        if host:
            t0 = time.perf_counter()
            table, u, lk = kc.export(), kc.unitigs(1, 0), kc.unitig_links(1, 0)
            t1 = time.perf_counter()
            h_lo, h_cnt, h_v, h_words = host_clean(table, u, lk, k, bool(canonical), tip, isl)
            t2 = time.perf_counter()
            out.update(host_export_ms=(t1 - t0) * 1e3, host_numpy_ms=(t2 - t1) * 1e3)
            rd = lambda p, nbytes: kd.device_view(p, (nbytes + 7) // 8, dev).cpu().numpy().view(np.uint8)[:nbytes].copy()
            dh, dl, dc, dv, nk, nu, summ = kc.clean_unitigs_device(1, 0, tip, isl)
            out["host_equal"] = bool(summ.words() == h_words and np.array_equal(rd(dl, 8 * nk).view(U64), h_lo) and
                                     np.array_equal(rd(dc, 8 * nk).view(U64), h_cnt) and np.array_equal(rd(dv, nu), h_v))
        kc.close()
    print(json.dumps(out), flush=True)


def parse(line):
    return {name: float(val) if "." in val else int(val) for name, val in re.findall(r"(\w+) ([\d.]+)", line.split(":", 1)[1])}


def measure(args, pool, canonical, gb, k=31):
    env = dict(os.environ, KMC_UNITIG_TRACE="1")
    cmd = [sys.executable, os.path.abspath(__file__), "--child", f"{pool},{int(canonical)},{k},{args.tip_keys},{args.island_keys}", "--gb", str(gb),
           "--reps", str(args.reps)] + (["--no-host"] if args.no_host else [])
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    if r.returncode:                            # nothing more is started on a device where a process has just failed
        raise RuntimeError("the traced child failed (exit %d): %s" % (r.returncode, r.stderr[-400:]))
    res = json.loads(r.stdout.strip().splitlines()[-1])
    sect, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("mark "):
            cur = line[5:]
            sect[cur] = []
        elif cur and line.split(":")[0] in ("kmc_unitigs", "kmc_unitig_links", "kmc_unitig_clean"):
            sect[cur].append(line)
    assert all(l.startswith("kmc_unitig_clean:") for l in sect["clean"] + sect["rounds"]), "the unitigs and links were not reused"
    ms = [parse(l)["clean_ms"] for l in sect["clean"]]
    assert len(ms) == args.reps
    n, kept = res["keys"], res["summary"][3]
    med = float(np.median(ms))
    # what the pass must move: the view's keys and counts once, the kept entries written (one-word keys).  A LOWER BOUND of what
    # it does move: on top, the mark pass reads adj (2 bytes), the ranking entry (8) and the count (8) of every row and writes
    # a class byte, the scatter pass reads that byte, and key and count of a kept row once more.  Left out: the uid_of (4 bytes) and verdict
    # (1 byte) gathers per solid row, the verdict kernel's reads, the tile counts and their scan.
    must = 16 * n + 16 * kept
    model = n * (2 + 8 + 8 + 1) + n + 32 * kept
    row = dict(table=f"pool{pool}_k{k}_{'canonical' if canonical else 'forward'} ({gb:g} GB, {n} keys)", n=n, limits=[args.tip_keys, args.island_keys],
               clean_ms_median=med, clean_ms_min=float(min(ms)), bytes_must_move=must, bytes_lower_bound_model=model, **res)
    if med:
        row["must_move_gbs"], row["model_gbs"] = must / med / 1e6, model / med / 1e6
        row["must_move_fraction_of_nominal"], row["model_fraction_of_nominal"] = row["must_move_gbs"] / NOMINAL_GBS, row["model_gbs"] / NOMINAL_GBS
        if row.get("read_peak_gbs"):
            row["must_move_fraction_of_measured"] = row["must_move_gbs"] / row["read_peak_gbs"]
            row["model_fraction_of_measured"] = row["model_gbs"] / row["read_peak_gbs"]
    if not args.no_host:
        assert row["host_equal"], "the host computation disagrees with the device"
        row["host_over_device"] = (row["host_export_ms"] + row["host_numpy_ms"]) / row["clean_ms_median"]
    return row


PASS = ("kmc_clean_verdict_kernel", "kmc_clean_mark_kernel", "kmc_scan_sums_kernel", "kmc_scan_top_kernel", "kmc_scan_final_kernel",
        "kmc_clean_scatter_kernel")


def split_from_trace(path):
    """Per-launch times of the clean pass from the kernel-trace CSV of a profiled --child run (rocprofv3 --kernel-trace
    --output-format csv -- python measure_clean.py --child ...): every dispatch of the verdict kernel that is followed by the
    five other launches of a pass, in order, is one pass; median microseconds per launch, of their sum, and of the span from
    the first launch's start to the last one's end (the difference is what the host spends between them)."""
    import csv
    with open(path, newline="") as f:
        rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f)))
    short = lambda name: next((p for p in PASS if p in name), None)
    seq = [(a, b, short(name)) for a, b, name in rows]
    passes = []
    for i in range(len(seq) - len(PASS) + 1):
        win = seq[i:i + len(PASS)]
        if tuple(w[2] for w in win) == PASS:
            passes.append(win)
    assert passes, "no clean pass in the trace"
    out = {"passes": len(passes)}
    for j, name in enumerate(PASS):
        out[name + "_us"] = float(np.median([(w[j][1] - w[j][0]) / 1e3 for w in passes]))
    out["kernels_sum_us"] = float(np.median([sum(b - a for a, b, _ in w) / 1e3 for w in passes]))
    out["span_us"] = float(np.median([(w[-1][1] - w[0][0]) / 1e3 for w in passes]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=1.0, help="FASTA size of the pool-10 input")
    ap.add_argument("--gb-distinct", type=float, default=0.05, help="FASTA size of the all-distinct input")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pools", default="10,0")
    ap.add_argument("--tip-keys", type=int, default=31)
    ap.add_argument("--island-keys", type=int, default=31)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy comparison")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--out", default="")
    ap.add_argument("--split-from-trace", default="", help="a kernel-trace CSV of a profiled --child run: print the per-launch split and stop")
    args = ap.parse_args()
    if args.split_from_trace:
        print(json.dumps(split_from_trace(args.split_from_trace)))
        return
    if args.child:
        child(args.child, args.gb, args.reps, not args.no_host)
        return
    rows = []
    for pool in [int(x) for x in args.pools.split(",")]:
        for canonical in (True, False):
            row = measure(args, pool, canonical, args.gb if pool else args.gb_distinct)
            print(json.dumps(row), flush=True)
            rows.append(row)
            if args.out:
                with open(args.out, "w") as f:
                    json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
