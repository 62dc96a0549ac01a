#!/usr/bin/env python3
"""Time the links pass of kmc_unitig_links_device beside the phases of the unitig call it follows.

Tables, k = 31, canonical and forward: the benchmark's pool-10 generator input (a few thousand keys), a pool-1000 input
(--gb GB of FASTA each) and synth pool 0 (every line fresh random: all-distinct, --gb-distinct GB).  Per table and range, in
a child process with KMC_UNITIG_TRACE set so that the library prints its own event times:
  * one warm kmc_unitigs_device call: its phases (adj_ms is the one the links pass is compared with: the same kind of
    lookups, for every row instead of for the rows with a terminal side) and their sum;
  * --reps kmc_unitig_links_device calls behind it, which find the unitigs in the ctx and run the links pass alone:
    links_ms, median and minimum -- once with the resolved targets kept in the per-row scratch (the default) and once with
    KMC_LINKS_LOOKUP_TWICE set, which makes the fill pass repeat the lookups;
  * the same calls timed from outside with event pairs on the ctx's stream (host waits included).
The two variants must give the same arrays.  One JSON line per measurement on stdout; --out also writes them to a file."""
import argparse
import importlib
import json
import os
import re
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

kmc = importlib.import_module("k-mer-count_amd")
kd = importlib.import_module("k-mer-count_amd.distributed")


def make_ctx(gb, pool, canonical, k, stream, dev):
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


def ev_ms(stream, f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    f()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def dev_words(ptr, n_bytes, dev):
    if not n_bytes:
        return np.zeros(0, np.uint8)
    return kd.device_view(ptr, (n_bytes + 7) // 8, dev).cpu().numpy().view(np.uint8)[:n_bytes].copy()


def child(spec, gb, reps):
    """one table, one range: the calls whose trace lines the parent reads; event times and the summary on stdout"""
    pool, canonical, k, lo_c, hi_c = [int(x) for x in spec.split(",")]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    out = {}
    with torch.cuda.stream(stream):
        kc, nd = make_ctx(gb, pool, bool(canonical), k, stream, dev)
        os.environ.pop("KMC_UNITIG_TRACE", None)
        kc.unitigs_device(lo_c, hi_c)              # warm: buffers and the index exist
        kc.unitig_links_device(lo_c, hi_c)
        os.environ["KMC_UNITIG_TRACE"] = "1"
        print("mark unitigs", file=sys.stderr, flush=True)
        out["unitigs_call_ms"] = ev_ms(stream, lambda: kc.unitigs_device(lo_c, hi_c))
        arrays = {}
        for name, twice in (("scratch", False), ("lookup_twice", True)):
            if twice:
                os.environ["KMC_LINKS_LOOKUP_TWICE"] = "1"
            else:
                os.environ.pop("KMC_LINKS_LOOKUP_TWICE", None)
            kc.unitig_links_device(lo_c, hi_c)     # (the scratch variant allocates its scratch on its first call)
            print("mark " + name, file=sys.stderr, flush=True)
            res = {}
            ms = [ev_ms(stream, lambda: res.update(r=kc.unitig_links_device(lo_c, hi_c))) for _ in range(reps)]
            do, dt, nu, nl, summ = res["r"]
            arrays[name] = (dev_words(do, 8 * (2 * nu + 1), dev), dev_words(dt, 4 * nl, dev))
            out[name + "_call_ms_median"], out[name + "_call_ms_min"] = float(np.median(ms)), float(min(ms))
            out["summary"] = summ.words()
        print("mark end", file=sys.stderr, flush=True)
        out["variants_equal"] = all(np.array_equal(a, b) for a, b in zip(arrays["scratch"], arrays["lookup_twice"]))
        out["keys"] = nd
        kc.close()
    print(json.dumps(out), flush=True)


def parse(line):
    return {name: float(val) if "." in val else int(val) for name, val in re.findall(r"(\w+) ([\d.]+)", line.split(":", 1)[1])}


def measure(args, pool, canonical, gb, lo_c, hi_c, k=31):
    env = dict(os.environ, KMC_UNITIG_TRACE="1")
    env.pop("KMC_LINKS_LOOKUP_TWICE", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", f"{pool},{int(canonical)},{k},{lo_c},{hi_c}", "--gb", str(gb),
                        "--reps", str(args.reps)], capture_output=True, text=True, env=env)
    if r.returncode:                            # nothing more is started on a device where a process has just failed
        raise RuntimeError("the traced child failed (exit %d): %s" % (r.returncode, r.stderr[-400:]))
    res = json.loads(r.stdout.strip().splitlines()[-1])
    sect, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("mark "):
            cur = line[5:]
            sect[cur] = []
        elif cur and (line.startswith("kmc_unitigs:") or line.startswith("kmc_unitig_links:")):
            sect[cur].append(line)
    phases = parse([l for l in sect["unitigs"] if l.startswith("kmc_unitigs:")][-1])
    row = dict(table=f"pool{pool}_k{k}_{'canonical' if canonical else 'forward'} ({gb:g} GB, {res['keys']} keys)", range=[lo_c, hi_c],
               n=res["keys"], summary=res["summary"], unitigs_phases=phases,
               unitigs_ms=sum(v for n, v in phases.items() if n.endswith("_ms")), adj_ms=phases.get("adj_ms"),
               unitigs_call_ms=res["unitigs_call_ms"], variants_equal=res["variants_equal"])
    for name in ("scratch", "lookup_twice"):
        ms = [parse(l)["links_ms"] for l in sect[name] if l.startswith("kmc_unitig_links:")]
        assert len(ms) == args.reps and all("unitigs_reused 1" in l for l in sect[name]), sect[name]
        row[name] = dict(links_ms_median=float(np.median(ms)), links_ms_min=float(min(ms)), call_ms_median=res[name + "_call_ms_median"],
                         call_ms_min=res[name + "_call_ms_min"])
    row["links_over_adj"] = row["scratch"]["links_ms_median"] / row["adj_ms"] if row["adj_ms"] else None
    assert row["variants_equal"], "the two variants of the fill pass disagree"
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=1.0, help="FASTA size of the pool-10 and pool-1000 inputs")
    ap.add_argument("--gb-distinct", type=float, default=0.05, help="FASTA size of the all-distinct input")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pools", default="10,1000,0")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.child:
        child(args.child, args.gb, args.reps)
        return
    rows = []
    for pool in [int(x) for x in args.pools.split(",")]:
        for canonical in (True, False):
            for lo_c, hi_c in ((1, 0), (2, 0)):
                row = measure(args, pool, canonical, args.gb if pool else args.gb_distinct, lo_c, hi_c)
                print(json.dumps(row), flush=True)
                rows.append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
