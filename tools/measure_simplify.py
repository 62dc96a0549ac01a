#!/usr/bin/env python3
"""Time the simplify pass of kmc_unitig_simplify_device beside the clean pass it extends, on three kinds of table.

(a) Tables without bubbles: synth pool 0 (every line fresh random: all-distinct; --gb-distinct 0.05 gives the 41.85 M-key
    tables of §4.13), k = 31, canonical and forward.  In one child process, behind one kmc_unitig_links_device call: --reps
    kmc_unitig_clean_device calls with limits 31 / 31 and --reps kmc_unitig_simplify_device calls with 31 / 31 / 31.  Both
    find the unitigs and links in the ctx, so each trace line times its pass alone; the difference is the price of the
    candidate test where nothing is a candidate.  The device's read peak is taken as tools/measure_clean.py takes it.
(b) A table with bubbles at size, built here: a seeded random genome of --genome bases read three times in reads of 1000
    and, every --every bases, one read of 2k - 1 bases with its middle base changed.  The pass time, the bubbles popped,
    one full round (kmc_unitig_simplify_into a fresh ctx and its kmc_finalize, wall time), and the same answer from
    kmc_export + kmc_unitigs + kmc_unitig_links with numpy (tests/bubble_model.np_simplify, which tests/test_simplify_host.py
    checks against the model), timed and compared for equality.
(c) The benchmark's pool-10 generator input (--gb GB of FASTA, a few thousand keys): the floor of a call.
Per table a child process with KMC_UNITIG_TRACE set, so that the library prints its own event times; one JSON line per
table on stdout, --out also writes them to a file.  The byte model is §4.13's: what the pass must move is the view's keys
and counts once and the kept entries written."""
import argparse
import importlib
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

U64 = np.uint64
NOMINAL_GBS = 8000.0   # the HBM peak §4.7 quotes its fractions against


def bubble_reads(genome_bases, every, k, seed):
    """(bases, offsets) of the genome's reads -- 1000 bases each, overlapping by k - 1 -- and (bases, offsets) of the
    substitution reads, one per `every` bases"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 4, genome_bases).astype(np.uint8)
    code = np.frombuffer(b"ACGT", np.uint8)
    step = 1000 - (k - 1)
    starts = np.arange(0, genome_bases - k, step)
    ends = np.minimum(starts + 1000, genome_bases)
    lens = ends - starts
    idx = np.repeat(starts, lens) + (np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens))
    offs = np.zeros(len(starts) + 1, U64)
    offs[1:] = np.cumsum(lens)
    p = np.arange(k, genome_bases - k, every)
    sub = g[p[:, None] + np.arange(-(k - 1), k)[None, :]]
    sub[:, k - 1] = (sub[:, k - 1] + 1 + rng.integers(0, 3, len(p))) % 4
    s_offs = (np.arange(len(p) + 1) * (2 * k - 1)).astype(U64)
    return (code[g[idx]], offs), (code[sub.reshape(-1)], s_offs), len(p)


def child(spec, args):
    """one table: the calls whose trace lines the parent reads; everything else on stdout"""
    import torch
    kmc = importlib.import_module("k-mer-count_amd")
    kd = importlib.import_module("k-mer-count_amd.distributed")
    kind, canonical = spec.split(",")[0], bool(int(spec.split(",")[1]))
    k, reps = 31, args.reps
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    out = {}
    mark = lambda s: print("mark " + s, file=sys.stderr, flush=True)
    with torch.cuda.stream(stream):
        if kind == "bubbles":
            (gb_, go), (sb, so), n_sub = bubble_reads(args.genome, args.every, k, 1)
            kc = kmc.KmerCounter(k=k, canonical=canonical, stream=stream.cuda_stream)
            for _ in range(3):
                kc.add_batch(gb_, go)
            kc.add_batch(sb, so)
            nd = kc.finalize()[0]
            out["substitution_reads"] = n_sub
        else:
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import measure_clean
            kc, nd = measure_clean.make_ctx(kmc, torch, args.gb if kind == "pool10" else args.gb_distinct, 10 if kind == "pool10" else 0,
                                            canonical, k, stream, dev)
        kc.unitig_links_device(1, 0)
        kc.clean_unitigs_device(1, 0, k, k)               # warm: the buffers exist
        kc.simplify_unitigs_device(1, 0, k, k, k)
        mark("clean")
        for _ in range(reps):
            c_words = kc.clean_unitigs_device(1, 0, k, k)[6].words()
        mark("simplify")
        for _ in range(reps):
            dh, dl, dc, dv, nk, nu, summ = kc.simplify_unitigs_device(1, 0, k, k, k)
        out.update(keys=nd, clean_summary=c_words, summary=summ.words())
        mark("rounds")
        wall = []
        for _ in range(reps):
            dst = kmc.KmerCounter(k=k, canonical=canonical)
            t0 = time.perf_counter()
            kc.simplify_into(dst, 1, 0, k, k, k)
            n_dst = dst.finalize()[0]
            wall.append((time.perf_counter() - t0) * 1e3)
            dst.close()
        out.update(round_ms_median=float(np.median(wall)), round_ms_min=float(min(wall)), round_keys=n_dst)
        mark("end")
        if kind == "pool0":
            buf = torch.zeros(1 << 31, dtype=torch.uint8, device=dev)
            stream.synchronize()
            best = max((buf.numel() / kmc.read_peak_device(buf.data_ptr(), buf.numel(), 0, stream.cuda_stream, shape, 5)[0] / 1e6, shape)
                       for shape in range(4))
            out["read_peak_gbs"], out["read_peak_shape"] = best
            del buf
        if kind == "bubbles" and not args.no_host:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import bubble_model as bm
            t0 = time.perf_counter()
            table, u, lk = kc.export(), kc.unitigs(1, 0), kc.unitig_links(1, 0)
            t1 = time.perf_counter()
            h_lo, h_cnt, h_v, h_words = bm.np_simplify(table, u, lk, k, canonical, k, k, k)
            t2 = time.perf_counter()
            out.update(host_export_ms=(t1 - t0) * 1e3, host_numpy_ms=(t2 - t1) * 1e3)
            rd = lambda p, nbytes: kd.device_view(p, (nbytes + 7) // 8, dev).cpu().numpy().view(np.uint8)[:nbytes].copy()
            dh, dl, dc, dv, nk, nu, summ = kc.simplify_unitigs_device(1, 0, k, k, k)
            out["host_equal"] = bool(summ.words() == h_words and np.array_equal(rd(dl, 8 * nk).view(U64), h_lo) and
                                     np.array_equal(rd(dc, 8 * nk).view(U64), h_cnt) and np.array_equal(rd(dv, nu), h_v))
        kc.close()
    print(json.dumps(out), flush=True)


def parse(line):
    return {name: float(val) if "." in val else int(val) for name, val in re.findall(r"(\w+) ([\d.]+)", line.split(":", 1)[1])}


def measure(args, kind, canonical):
    env = dict(os.environ, KMC_UNITIG_TRACE="1")
    cmd = [sys.executable, os.path.abspath(__file__), "--child", f"{kind},{int(canonical)}", "--gb", str(args.gb), "--gb-distinct", str(args.gb_distinct),
           "--genome", str(args.genome), "--every", str(args.every), "--reps", str(args.reps)] + (["--no-host"] if args.no_host else [])
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    if r.returncode:                            # nothing more is started on a device where a process has just failed
        raise RuntimeError("the traced child failed (exit %d): %s" % (r.returncode, r.stderr[-400:]))
    res = json.loads(r.stdout.strip().splitlines()[-1])
    sect, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("mark "):
            cur = line[5:]
            sect[cur] = []
        elif cur and line.split(":")[0] in ("kmc_unitigs", "kmc_unitig_links", "kmc_unitig_clean", "kmc_unitig_simplify"):
            sect[cur].append(line)
    assert all(l.startswith("kmc_unitig_clean:") for l in sect["clean"]), "the unitigs and links were not reused"
    assert all(l.startswith("kmc_unitig_simplify:") for l in sect["simplify"] + sect["rounds"]), "the unitigs and links were not reused"
    c_ms, s_ms = [parse(l)["clean_ms"] for l in sect["clean"]], [parse(l)["clean_ms"] for l in sect["simplify"]]
    assert len(c_ms) == len(s_ms) == args.reps
    n, kept = res["keys"], res["summary"][3]
    med = float(np.median(s_ms))
    must = 16 * n + 16 * kept                   # §4.13's model: keys and counts read once, kept entries written (one-word keys)
    row = dict(table=f"{kind}_k31_{'canonical' if canonical else 'forward'} ({n} keys)", n=n, limits=[31, 31, 31],
               clean_ms_median=float(np.median(c_ms)), clean_ms_min=float(min(c_ms)), clean_ms_max=float(max(c_ms)),
               simplify_ms_median=med, simplify_ms_min=float(min(s_ms)), simplify_ms_max=float(max(s_ms)),
               simplify_minus_clean_ms=med - float(np.median(c_ms)), bytes_must_move=must, **res)
    if med:
        row["must_move_gbs"] = must / med / 1e6
        row["must_move_fraction_of_nominal"] = row["must_move_gbs"] / NOMINAL_GBS
        if row.get("read_peak_gbs"):
            row["must_move_fraction_of_measured"] = row["must_move_gbs"] / row["read_peak_gbs"]
    if "host_equal" in row:
        assert row["host_equal"], "the host computation disagrees with the device"
        row["host_over_device"] = (row["host_export_ms"] + row["host_numpy_ms"]) / med
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=0.1, help="FASTA size of the pool-10 input")
    ap.add_argument("--gb-distinct", type=float, default=0.05, help="FASTA size of the all-distinct input")
    ap.add_argument("--genome", type=int, default=4_000_000, help="bases of the genome of the table with bubbles")
    ap.add_argument("--every", type=int, default=300, help="one substitution read per this many bases")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tables", default="pool0,bubbles,pool10")
    ap.add_argument("--no-host", action="store_true", help="skip the numpy comparison")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.child:
        child(args.child, args)
        return
    rows = []
    for kind in args.tables.split(","):
        for canonical in (True, False):
            row = measure(args, kind, canonical)
            print(json.dumps(row), flush=True)
            rows.append(row)
            if args.out:
                with open(args.out, "w") as f:
                    json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
