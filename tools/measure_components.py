#!/usr/bin/env python3
"""Time the components pass of kmc_unitig_components_device on two kinds of table, beside the clean and
simplify passes on the same ctx.

(a) Tables where nearly every unitig is its own component: synth pool 0 (every line fresh random: all-distinct;
    --gb-distinct 0.05 gives the 41.85 M-key tables of §4.13), k = 31, canonical and forward.
(b) One giant component: the substitution-bubble table of tools/measure_simplify.py (a seeded random genome of --genome bases
    read three times and, every --every bases, one read of 2k - 1 bases with its middle base changed), BEFORE any simplify.
In one child process per table, behind one kmc_unitig_links_device call: --reps kmc_unitig_components_device calls with
limit k (each prints its trace line: the label rounds and the four phase times), --reps kmc_unitig_clean_device and --reps
kmc_unitig_simplify_device calls (the passes whose kernels the kept table shares; tools/measure_simplify.py times the same
two passes on a checkout from before the components calls), and the same answer on the host: kmc_unitigs +
kmc_unitig_links copied out and tests/components_model.np_components (which tests/test_components_host.py checks against
the model), timed and compared for equality.  That host time is the baseline the ratio is taken against.  One JSON line
per table on stdout; --out also writes them to a file under profiles/."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

U64, U32 = np.uint64, np.uint32
PHASES = ("label_ms", "number_ms", "stats_ms", "keep_ms")


def child(spec, args):
    """one table: the calls whose trace lines the parent reads; everything else on stdout"""
    import torch
    import measure_clean
    import measure_simplify
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
            (gb_, go), (sb, so), n_sub = measure_simplify.bubble_reads(args.genome, args.every, k, 1)
            kc = kmc.KmerCounter(k=k, canonical=canonical, stream=stream.cuda_stream)
            for _ in range(3):
                kc.add_batch(gb_, go)
            kc.add_batch(sb, so)
            nd = kc.finalize()[0]
            out["substitution_reads"] = n_sub
        else:
            kc, nd = measure_clean.make_ctx(kmc, torch, args.gb_distinct, 0, canonical, k, stream, dev)
        out["keys"] = nd
        kc.unitig_links_device(1, 0)
        kc.clean_unitigs_device(1, 0, k, k)               # warm: the buffers exist
        kc.simplify_unitigs_device(1, 0, k, k, k)
        kc.components_device(1, 0, k)
        mark("components")
        wall = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = kc.components_device(1, 0, k)
            wall.append((time.perf_counter() - t0) * 1e3)
        out.update(summary=r[9].words(), call_wall_ms_median=float(np.median(wall)), call_wall_ms_min=float(min(wall)))
        mark("clean")
        for _ in range(reps):
            out["clean_summary"] = kc.clean_unitigs_device(1, 0, k, k)[6].words()
        mark("simplify")
        for _ in range(reps):
            out["simplify_summary"] = kc.simplify_unitigs_device(1, 0, k, k, k)[6].words()
        mark("end")
        if not args.no_host:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import components_model as xm
            t0 = time.perf_counter()
            u, lk = kc.unitigs(1, 0), kc.unitig_links(1, 0)
            t1 = time.perf_counter()
            m = (np.diff(u.offsets.astype(np.int64)) - (k - 1)).astype(U64)
            h_comp, h_stats, h_verdict = xm.np_components(lk.offsets, lk.to, m, u.abund, k)
            t2 = time.perf_counter()
            out.update(host_export_ms=(t1 - t0) * 1e3, host_numpy_ms=(t2 - t1) * 1e3)
            rd = lambda p, nbytes: kd.device_view(p, (nbytes + 7) // 8, dev).cpu().numpy().view(np.uint8)[:nbytes].copy()
            dco, dst, dv, dh, dl, dc, nc, nu, nk, summ = kc.components_device(1, 0, k)
            out["host_equal"] = bool(np.array_equal(rd(dco, 4 * nu).view(U32), h_comp) and
                                     np.array_equal(rd(dst, 32 * nc).view(U64).reshape(nc, 4), h_stats) and np.array_equal(rd(dv, nu), h_verdict))
        kc.close()
    print(json.dumps(out), flush=True)


def parse(line):
    return {name: float(val) if "." in val else int(val) for name, val in re.findall(r"(\w+) ([\d.]+)", line.split(":", 1)[1])}


def spread(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


def measure(args, kind, canonical):
    env = dict(os.environ, KMC_UNITIG_TRACE="1")
    cmd = [sys.executable, os.path.abspath(__file__), "--child", f"{kind},{int(canonical)}", "--gb-distinct", str(args.gb_distinct),
           "--genome", str(args.genome), "--every", str(args.every), "--reps", str(args.reps)]
    cmd += ["--no-host"] if args.no_host else []
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    if r.returncode:                            # nothing more is started on a device where a process has just failed
        raise RuntimeError("the traced child failed (exit %d): %s" % (r.returncode, r.stderr[-400:]))
    res = json.loads(r.stdout.strip().splitlines()[-1])
    sect, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("mark "):
            cur = line[5:]
            sect[cur] = []
        elif cur and line.split(":")[0] in ("kmc_unitigs", "kmc_unitig_links", "kmc_unitig_clean", "kmc_unitig_simplify", "kmc_unitig_components"):
            sect[cur].append(line)
    assert all(l.startswith("kmc_unitig_clean:") for l in sect["clean"]), "the unitigs and links were not reused"
    assert all(l.startswith("kmc_unitig_simplify:") for l in sect["simplify"]), "the unitigs and links were not reused"
    row = dict(table=f"{kind}_k31_{'canonical' if canonical else 'forward'} ({res['keys']} keys)", limit=31,
               clean_ms=spread([parse(l)["clean_ms"] for l in sect["clean"]]),
               simplify_ms=spread([parse(l)["clean_ms"] for l in sect["simplify"]]), **res)
    assert all(l.startswith("kmc_unitig_components:") for l in sect["components"]), "the unitigs and links were not reused"
    lines = [parse(l) for l in sect["components"]]
    assert len(lines) == args.reps
    total = [sum(l[p] for p in PHASES) for l in lines]
    row.update(unitigs=lines[0]["unitigs"], records=lines[0]["records"], components=lines[0]["components"], rounds=sorted({l["rounds"] for l in lines}),
               components_ms=spread(total), **{p: spread([l[p] for l in lines]) for p in PHASES})
    row["host_polls"] = sorted({-(-l["rounds"] // 4) for l in lines})       # one synchronising copy per batch of four rounds
    if "host_equal" in row:
        assert row["host_equal"], "the host computation disagrees with the device"
        row["host_over_device"] = (row["host_export_ms"] + row["host_numpy_ms"]) / row["components_ms"]["median"]
        row["host_numpy_over_device"] = row["host_numpy_ms"] / row["components_ms"]["median"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb-distinct", type=float, default=0.05, help="FASTA size of the all-distinct input")
    ap.add_argument("--genome", type=int, default=4_000_000, help="bases of the genome of the table with bubbles")
    ap.add_argument("--every", type=int, default=300, help="one substitution read per this many bases")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tables", default="pool0,bubbles")
    ap.add_argument("--no-host", action="store_true", help="skip the numpy baseline")
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
