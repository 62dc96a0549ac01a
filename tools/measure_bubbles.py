#!/usr/bin/env python3
"""Time the bubbles pass of kmc_unitig_bubbles_device on the two tables of §4.14, canonical and forward.

(a) A table without candidates: synth pool 0 (every line fresh random: all-distinct; --gb-distinct 0.05 gives the 41.85 M-key
    tables of §4.13), k = 31.  The pair pass alone runs: what a call costs where there is nothing to report.
(b) The table with bubbles of tools/measure_simplify.py: a seeded random genome of --genome bases read three times and, every
    --every bases, one read of 2k - 1 bases with its middle base changed (4.41 M keys, 13 334 substitution bubbles with the
    defaults).  Every one of them has to be called, as a substitution, with lcp == k - 1.
Per table one child process with KMC_UNITIG_TRACE set, behind one kmc_unitig_links_device call: --reps
kmc_unitig_bubbles_device calls (their trace lines split the pass into pair_ms and diff_ms) and --reps
kmc_unitig_simplify_device calls with limits k / k / k (clean_ms).  With --parent-lib PATH the simplify calls are also timed
with that build of the library (a libkmc.so of the parent commit), --alternate times in turn with this one, each in a
process of its own: the parent's numbers are the yardstick for "simplify is as fast as it was", within their own spread.
On table (b) the same records are also made on the host from kmc_unitigs + kmc_unitig_links with numpy, timed and compared
word for word.  One JSON line per table on stdout, --out also writes them to a file."""
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

U64 = np.uint64
LINES = ("kmc_unitigs", "kmc_unitig_links", "kmc_unitig_clean", "kmc_unitig_simplify", "kmc_unitig_bubbles")


def host_records(unitigs, links, k, limit):
    """the records of kmc_unitig_bubbles from the host copies of the unitigs and links: candidates and called arms with
    tests/bubble_model.np_bubbles, the major arm over the at most four records of the end p, the difference per record"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bubble_model as bm
    import measure_clean as mc
    popped, cand = bm.np_bubbles(unitigs.offsets, unitigs.abund, unitigs.flags, links.offsets, links.to, k, limit)
    u = np.flatnonzero(popped)
    offs, abund = unitigs.offsets.astype(np.int64), unitigs.abund
    m = (np.diff(unitigs.offsets) - U64(k - 1)).astype(U64)
    lo = links.offsets.astype(np.int64)
    to = np.concatenate([links.to.astype(np.int64), [0]])
    nu = len(abund)
    p_all, q_all = to[lo[0:2 * nu:2]], to[lo[1:2 * nu:2]]
    p, q = p_all[u], q_all[u]
    best = np.full(len(u), -1, np.int64)
    for j in range(4):
        idx = lo[p] + j
        ok = idx < lo[p + 1]
        w = to[np.where(ok, idx, 0)] >> 1
        ok &= (w != u) & cand[w] & (((p_all[w] == p) & (q_all[w] == q)) | ((p_all[w] == q) & (q_all[w] == p)))
        b = np.where(best < 0, 0, best)
        lh, ll = mc._mul128(abund[w], m[b])
        rh, rl = mc._mul128(abund[b], m[w])
        more = (lh > rh) | ((lh == rh) & (ll > rl))
        same = (lh == rh) & (ll == rl)
        wins = more | (same & ((m[w] > m[b]) | ((m[w] == m[b]) & (w < b))))
        best = np.where(ok & ((best < 0) | wins), w, best)
    assert (best >= 0).all()
    rev = to[lo[2 * best]] != p
    comp = np.zeros(256, np.uint8)
    comp[[ord(c) for c in "ACGT"]] = [ord(c) for c in "TGCA"]
    rec = np.zeros((len(u), 8), np.uint32)
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3] = u, best, p, q
    bases = unitigs.bases
    for i in range(len(u)):
        U, W = bases[offs[u[i]]:offs[u[i] + 1]], bases[offs[best[i]]:offs[best[i] + 1]]
        if rev[i]:
            W = comp[W[::-1]]
        n = min(len(U), len(W))
        ne = U[:n] != W[:n]
        lcp = int(np.argmax(ne)) if ne.any() else n
        cap = n - lcp
        ns = U[len(U) - cap:][::-1] != W[len(W) - cap:][::-1]
        lcs = int(np.argmax(ns)) if ns.any() else cap
        mism = int(ne.sum()) if len(U) == len(W) else 0
        kind = 0 if len(U) == len(W) and mism == 1 else 1 if (len(U) - lcp - lcs == 0) != (len(W) - lcp - lcs == 0) else 2
        rec[i, 4:] = lcp, lcs, kind | (4 if rev[i] else 0), mism
    return rec, int(cand.sum())


def child(spec, args):
    """one table: the calls whose trace lines the parent reads; everything else on stdout"""
    import torch
    kmc = importlib.import_module("k-mer-count_amd")
    kd = importlib.import_module("k-mer-count_amd.distributed")
    import measure_clean
    import measure_simplify
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
        kc.simplify_unitigs_device(1, 0, k, k, k)               # warm: the buffers exist
        if not args.simplify_only:
            kc.bubbles_device(1, 0, k)
            mark("bubbles")
            for _ in range(reps):
                d, nr, nu, summ = kc.bubbles_device(1, 0, k)
            out.update(summary=summ.words(), records=nr)
            rec = kd.device_view(d, max(4 * nr, 1), dev).cpu().numpy().view(np.uint32)[:8 * nr].reshape(nr, 8).copy()
            out["all_subst_lcp_k_minus_1"] = bool(nr and (rec[:, 6] & 3 == 0).all() and (rec[:, 4] == k - 1).all() and (rec[:, 5] == k - 1).all())
        mark("simplify")
        for _ in range(reps):
            s_words = kc.simplify_unitigs_device(1, 0, k, k, k)[6].words()
        out["simplify_summary"] = s_words
        mark("end")
        if kind == "bubbles" and not args.no_host and not args.simplify_only:
            t0 = time.perf_counter()
            u, lk = kc.unitigs(1, 0), kc.unitig_links(1, 0)
            t1 = time.perf_counter()
            h_rec, h_cand = host_records(u, lk, k, k)
            t2 = time.perf_counter()
            out.update(host_export_ms=(t1 - t0) * 1e3, host_numpy_ms=(t2 - t1) * 1e3,
                       host_equal=bool(np.array_equal(h_rec, rec) and h_cand == summ.words()[2]))
        kc.close()
    print(json.dumps(out), flush=True)


def parse(line):
    return {name: float(val) if "." in val else int(val) for name, val in re.findall(r"(\w+) ([\d.]+)", line.split(":", 1)[1])}


def run_child(args, kind, canonical, lib=None):
    """(the child's JSON, {mark: its trace lines})"""
    env = dict(os.environ, KMC_UNITIG_TRACE="1")
    if lib:
        env["KMC_LIB_PATH"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", f"{kind},{int(canonical)}", "--gb-distinct", str(args.gb_distinct),
           "--genome", str(args.genome), "--every", str(args.every), "--reps", str(args.reps)]
    cmd += (["--no-host"] if args.no_host else []) + (["--simplify-only"] if lib else [])
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    if r.returncode:                            # nothing more is started on a device where a process has just failed
        raise RuntimeError("the traced child failed (exit %d): %s" % (r.returncode, r.stderr[-400:]))
    sect, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("mark "):
            cur = line[5:]
            sect[cur] = []
        elif cur and line.split(":")[0] in LINES:
            sect[cur].append(line)
    return json.loads(r.stdout.strip().splitlines()[-1]), sect


def spread(ms):
    return dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)))


def measure(args, kind, canonical):
    res, sect = run_child(args, kind, canonical)
    assert all(l.startswith("kmc_unitig_bubbles:") for l in sect["bubbles"]), "the unitigs and links were not reused"
    assert all(l.startswith("kmc_unitig_simplify:") for l in sect["simplify"]), "the unitigs and links were not reused"
    pair, diff = [parse(l)["pair_ms"] for l in sect["bubbles"]], [parse(l)["diff_ms"] for l in sect["bubbles"]]
    simp = [[parse(l)["clean_ms"] for l in sect["simplify"]]]
    assert len(pair) == len(simp[0]) == args.reps
    parent = []
    for _ in range(args.alternate if args.parent_lib else 0):
        _, s = run_child(args, kind, canonical, args.parent_lib)
        parent.append([parse(l)["clean_ms"] for l in s["simplify"]])
        _, s = run_child(args, kind, canonical, os.path.join(ROOT, "k-mer-count_amd", "libkmc.so"))
        simp.append([parse(l)["clean_ms"] for l in s["simplify"]])
    n = res["keys"]
    row = dict(table=f"{kind}_k31_{'canonical' if canonical else 'forward'} ({n} keys)", n=n, limit=31, pair_ms=spread(pair), diff_ms=spread(diff),
               bubbles_ms_median=float(np.median(np.array(pair) + np.array(diff))), simplify_ms=[spread(x) for x in simp],
               simplify_parent_ms=[spread(x) for x in parent], **res)
    if kind == "bubbles":
        assert res["records"] == res["substitution_reads"] == res["summary"][3] and res["all_subst_lcp_k_minus_1"], res
        assert res["summary"][1] == res["simplify_summary"][8] and res["summary"][2] == res["simplify_summary"][10]
    else:
        assert res["records"] == 0
    if "host_equal" in row:
        assert row["host_equal"], "the host computation disagrees with the device"
        row["host_over_device"] = (row["host_export_ms"] + row["host_numpy_ms"]) / row["bubbles_ms_median"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb-distinct", type=float, default=0.05, help="FASTA size of the all-distinct input")
    ap.add_argument("--genome", type=int, default=4_000_000, help="bases of the genome of the table with bubbles")
    ap.add_argument("--every", type=int, default=300, help="one substitution read per this many bases")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tables", default="pool0,bubbles")
    ap.add_argument("--parent-lib", default="", help="a libkmc.so of the parent commit: its simplify pass is timed in turn with this one's")
    ap.add_argument("--alternate", type=int, default=2, help="how often the two libraries take turns")
    ap.add_argument("--no-host", action="store_true", help="skip the numpy comparison")
    ap.add_argument("--simplify-only", action="store_true", help=argparse.SUPPRESS)
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
