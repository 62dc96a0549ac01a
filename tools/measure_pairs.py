#!/usr/bin/env python3
"""Time kmc_unitig_pairs_device: the map passes it runs, the anchor and pair passes, the sort and the reduce
pass, beside what they are compared with.

Tables, k = 31, canonical and forward:
(a) pool0: synth pool 0 (every line fresh random: all-distinct; --gb-distinct 0.05 gives the 41.85 M-key tables of the other
    view rows), the counted batch taken two reads at a time.  Every read is a unitig of its own: every pair is a record.
(b) bubbles: the table with bubbles of tools/measure_simplify.py (4.41 M keys, 40 003 unitigs with the defaults), its own
    reads taken two at a time.
(c) hot: the `hot` input of tests/pair_inputs.py -- 1000 pairs on ONE record -- repeated until the batch has as many reads as
    table (b)'s (--hot-reads to ask for more): every lane adds to the same three words.
Per table one child process with KMC_UNITIG_TRACE set, behind one warm call of each kind: --reps kmc_unitig_pairs_device
calls (their trace lines give map_ms, anchor_ms, sort_ms, reduce_ms), the same with KMC_PAIRS_PLAIN set (every lane issues its
own atomics: the A/B behind the LDS table; both must give the same arrays), and --reps kmc_unitig_map_device and
kmc_unitig_transits_device calls on the same batch.  On (b) and (c) the same arrays are also made on the host from
kmc_unitig_map + the unitig offsets with numpy, timed and compared word for word.  With --parent-lib PATH (a libkmc.so of
the parent commit) the map and transits calls are also timed with that build, --alternate times in turn with this one, each
in a process of its own: they run no new code, so they have to stay inside the parent's own run-to-run spread.  (bench.py is
not run from here: it is started by hand with KMC_LIB_PATH naming the parent's library and without it, in turns.)  One JSON
line per table on stdout, --out also writes them to a file."""
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

from measure_transits import bubble_read_count, ev_ms, parse, spread  # noqa: E402

U64, I64 = np.uint64, np.int64
LINES = ("kmc_unitigs", "kmc_unitig_links", "kmc_unitig_map", "kmc_unitig_transits", "kmc_unitig_pairs")
NAMES = ("pair_class", "pair_ends", "pair_value", "rec_ends", "rec_count", "rec_sum", "rec_min", "rec_max", "insert_hist")


def host_pairs(segs, seg_offsets, u_offsets, k, n_bins):
    """the nine arrays and the summary from the host copies of a map result and the unitig offsets, by the definitions of
    include/kmc.h, vectorised over the reads"""
    so = seg_offsets.astype(I64)
    n_reads = len(so) - 1
    ns = len(segs)
    ln = segs[:, 1].astype(I64)
    read_of = np.repeat(np.arange(n_reads), np.diff(so))
    # the longest segment of a read, of equally long ones the last: the greatest (len, index)
    best = np.full(n_reads, -1, I64)
    if ns:
        order = np.lexsort((np.arange(ns), ln, read_of))
        last = np.flatnonzero(np.r_[read_of[order][1:] != read_of[order][:-1], True])
        best[read_of[order][last]] = order[last]
    has = best >= 0
    b = np.where(has, best, 0)
    if ns:
        start, uni, pos = segs[b, 0].astype(I64), segs[b, 2].astype(I64), segs[b, 3].astype(I64)
    else:
        start = uni = pos = np.zeros(n_reads, I64)
    u, o = uni >> 1, uni & 1
    L = np.diff(u_offsets.astype(I64)) if len(u_offsets) > 1 else np.zeros(1, I64)
    Lu = L[np.where(has, u, 0)]
    m = Lu - (k - 1)
    reach = start + np.where(o == 1, pos + 1, m - pos) + k - 1
    e = np.where(has, 2 * u + 1 - o, 0xFFFFFFFF)
    eA, eB, hA, hB = e[0::2], e[1::2], has[0::2], has[1::2]
    uA, uB, R, LA = u[0::2], u[1::2], reach[0::2] + reach[1::2], Lu[0::2]
    both = hA & hB
    span = both & (uA != uB)
    opp = both & (uA == uB) & (((eA ^ eB) & 1) == 1)
    proper = opp & (R > LA)
    cls = np.where(~both, 0, np.where(span, 1, np.where(proper, 2, np.where(opp, 3, 4)))).astype(np.uint8)
    value = np.where(span, R, np.where(proper, R - LA, 0)).astype(U64)
    ends = np.stack([eA, eB], 1).astype(np.uint32).reshape(-1)
    hist = np.bincount(np.minimum(value[proper].astype(I64), n_bins - 1), minlength=n_bins).astype(U64)
    a, bb = np.minimum(eA, eB)[span], np.maximum(eA, eB)[span]
    key = (a.astype(U64) << U64(32)) | bb.astype(U64)
    keys, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    Rs = R[span].astype(U64)
    rsum, rmin, rmax = np.zeros(len(keys), U64), np.full(len(keys), ~U64(0), U64), np.zeros(len(keys), U64)
    np.add.at(rsum, inv, Rs)
    np.minimum.at(rmin, inv, Rs)
    np.maximum.at(rmax, inv, Rs)
    rec_ends = np.stack([keys >> U64(32), keys & U64(0xFFFFFFFF)], 1).astype(np.uint32).reshape(-1)
    summary = [len(cls)] + [int((cls == c).sum()) for c in range(5)] + [len(keys), int(value[proper].sum())]
    return (cls, ends, value, rec_ends, cnt.astype(U64), rsum, rmin, rmax, hist), summary


def child(spec, args):
    """one table: the calls whose trace lines the parent reads; everything else on stdout"""
    import torch
    kmc = importlib.import_module("k-mer-count_amd")
    kd = importlib.import_module("k-mer-count_amd.distributed")
    import measure_simplify
    kind, canonical = spec.split(",")[0], bool(int(spec.split(",")[1]))
    k, reps, bins = 31, args.reps, args.bins
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    out = {}
    mark = lambda s: print("mark " + s, file=sys.stderr, flush=True)

    def upload(bases, offs):
        d_b = torch.zeros(len(bases) + 64, dtype=torch.uint8, device=dev)
        d_b[:len(bases)] = torch.from_numpy(np.ascontiguousarray(bases))
        d_o = torch.from_numpy(np.ascontiguousarray(offs).view(np.int64).copy()).to(dev)
        return d_b, d_o

    with torch.cuda.stream(stream):
        kc = kmc.KmerCounter(k=k, canonical=canonical, stream=stream.cuda_stream)
        bases = offs = None
        if kind == "pool0":
            s = kmc.Synth(seed=1, pool=0)
            n_reads, _ = kmc.synth_records_for_bytes(s, int(args.gb_distinct * 1e9))
            n_reads -= n_reads & 1
            n_bases = n_reads * s.read_len
            d_b = torch.zeros(n_bases + 64, dtype=torch.uint8, device=dev)
            d_o = torch.empty(n_reads + 1, dtype=torch.int64, device=dev)
            kmc.synth_reads_device(s, 0, n_reads, d_b.data_ptr(), d_o.data_ptr(), 0, stream.cuda_stream)
            stream.synchronize()
            kc.add_batch_device(d_b.data_ptr(), d_o.data_ptr(), n_reads, n_bases, s.read_len)
        elif kind == "bubbles":
            (gb_, go), (sb, so), _ = measure_simplify.bubble_reads(args.genome, args.every, k, 1)
            for _ in range(3):
                kc.add_batch(gb_, go)
            kc.add_batch(sb, so)
            bases, offs = np.concatenate([gb_, sb]), np.concatenate([go, so[1:] + go[-1]]).astype(U64)
            n_reads = (len(offs) - 1) & ~1
            offs = offs[:n_reads + 1]
            bases = bases[:int(offs[-1])]
            n_bases = len(bases)
            d_b, d_o = upload(bases, offs)
        else:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import map_inputs
            import pair_inputs
            sample, pairs = pair_inputs.hot(k, 730, 1000)
            kc.add_batch(*map_inputs.pack(sample))
            one_b, one_o = map_inputs.pack(pair_inputs.reads_of(pairs))
            copies = -(-(args.hot_reads or bubble_read_count(args)) // (len(one_o) - 1))
            bases = np.tile(one_b, copies)
            offs = np.concatenate([[0], (one_o[1:][None, :] + (np.arange(copies, dtype=U64) * U64(len(one_b)))[:, None]).ravel()]).astype(U64)
            n_reads, n_bases = len(offs) - 1, len(bases)
            d_b, d_o = upload(bases, offs)
            out["copies"] = copies
        torch.cuda.synchronize(dev)
        out["keys"] = kc.finalize()[0]
        batch = (d_b.data_ptr(), d_o.data_ptr(), n_reads, n_bases)
        os.environ.pop("KMC_PAIRS_PLAIN", None)
        kc.transits_device(*batch, 1, 0)             # warm: the buffers, the links, the prefix index and the row index exist
        kc.map_reads_device(*batch, 1, 0)
        arrays = {}
        if not args.base_only:
            kc.pair_links_device(*batch, 1, 0, bins)
            for name, plain in (("pairs", False), ("plain", True)):
                if plain:
                    os.environ["KMC_PAIRS_PLAIN"] = "1"
                mark("warm")
                kc.pair_links_device(*batch, 1, 0, bins)
                mark(name)
                res = {}
                out[name + "_call_ms"] = [ev_ms(torch, stream, lambda: res.update(r=kc.pair_links_device(*batch, 1, 0, bins))) for _ in range(reps)]
                *p, n_pairs, nr, summ = res["r"]
                words = lambda ptr, n: kd.device_view(ptr, max((n + 7) // 8, 1), dev).cpu().numpy().view(np.uint8)[:n].copy()
                arrays[name] = (words(p[0], n_pairs), words(p[1], 8 * n_pairs).view(np.uint32), words(p[2], 8 * n_pairs).view(U64),
                                words(p[3], 8 * nr).view(np.uint32)) + tuple(words(p[i], 8 * nr).view(U64) for i in (4, 5, 6, 7)) + (words(p[8], 8 * bins).view(U64),)
                out.update(summary=summ.words(), pairs=n_pairs, records=nr)
            os.environ.pop("KMC_PAIRS_PLAIN", None)
            out["variants_equal"] = all(np.array_equal(x, y) for x, y in zip(arrays["pairs"], arrays["plain"]))
        mark("map")
        out["map_call_ms"] = [ev_ms(torch, stream, lambda: kc.map_reads_device(*batch, 1, 0)) for _ in range(reps)]
        mark("transits")
        out["transits_call_ms"] = [ev_ms(torch, stream, lambda: kc.transits_device(*batch, 1, 0)) for _ in range(reps)]
        mark("end")
        out.update(reads=n_reads, bases=n_bases)
        if bases is not None and not args.no_host and not args.base_only:
            os.environ.pop("KMC_UNITIG_TRACE", None)
            t0 = time.perf_counter()
            m, u = kc.map_reads(bases, offs, 1, 0), kc.unitigs(1, 0)
            t1 = time.perf_counter()
            host, hsum = host_pairs(m.segments, m.seg_offsets, u.offsets, k, bins)
            t2 = time.perf_counter()
            bad = [n for n, x, y in zip(NAMES, host, arrays["pairs"]) if not np.array_equal(x, y)]
            out.update(host_export_ms=(t1 - t0) * 1e3, host_numpy_ms=(t2 - t1) * 1e3, host_equal=bool(not bad and hsum == out["summary"]), host_differs=bad)
        kc.close()
    print(json.dumps(out), flush=True)


def run_child(args, kind, canonical, lib=None):
    """(the child's JSON, {mark: its trace lines})"""
    env = dict(os.environ, KMC_UNITIG_TRACE="1")
    env.pop("KMC_PAIRS_PLAIN", None)
    if lib:
        env["KMC_LIB_PATH"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", f"{kind},{int(canonical)}", "--gb-distinct", str(args.gb_distinct),
           "--genome", str(args.genome), "--every", str(args.every), "--reps", str(args.reps), "--hot-reads", str(args.hot_reads), "--bins", str(args.bins)]
    cmd += (["--no-host"] if args.no_host else []) + (["--base-only"] if lib else [])
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    if r.returncode:                            # nothing more is started on a device where a process has just failed
        raise RuntimeError("the traced child failed (exit %d): %s" % (r.returncode, r.stderr[-600:]))
    sect, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("mark "):
            cur = line[5:]
            sect[cur] = []
        elif cur and line.split(":")[0] in LINES:
            sect[cur].append(line)
    return json.loads(r.stdout.strip().splitlines()[-1]), sect


def base_times(sect):
    """(map: index + place + segs per call, transits: transit + verdict per call) of a child's map and transits sections"""
    maps = [parse(l) for l in sect["map"] if l.startswith("kmc_unitig_map:")]
    trs = [parse(l) for l in sect["transits"] if l.startswith("kmc_unitig_transits:")]
    return [m["index_ms"] + m["place_ms"] + m["segs_ms"] for m in maps], [t["map_ms"] + t["transit_ms"] + t["verdict_ms"] for t in trs]


def transit_parts(sect):
    """the medians of the three phases of the transits calls of a child, for a figure that needs explaining"""
    trs = [parse(l) for l in sect["transits"] if l.startswith("kmc_unitig_transits:")]
    return {f: float(np.median([t[f] for t in trs])) for f in ("map_ms", "transit_ms", "verdict_ms")}


def measure(args, kind, canonical):
    res, sect = run_child(args, kind, canonical)
    row = dict(table=f"{kind}_k31_{'canonical' if canonical else 'forward'} ({res['keys']} keys)", **res)
    passes = ("map_ms", "anchor_ms", "sort_ms", "reduce_ms")
    for name in ("pairs", "plain"):
        lines = [parse(l) for l in sect[name] if l.startswith("kmc_unitig_pairs:")]
        assert len(lines) == args.reps and all(l["unitigs_reused"] == 1 for l in lines), sect[name]
        row[name] = {f: spread([l[f] for l in lines]) for f in passes}
    for f in passes[1:]:
        row[f.replace("_ms", "_share_of_map")] = row["pairs"][f]["median"] / row["pairs"]["map_ms"]["median"]
    row["plain_over_table"] = row["plain"]["reduce_ms"]["median"] / row["pairs"]["reduce_ms"]["median"]
    maps, trs = base_times(sect)
    row["map_ms"], row["transits_ms"] = [spread(maps)], [spread(trs)]
    row["map_parent_ms"], row["transits_parent_ms"] = [], []
    row["transits_parts_ms"], row["transits_parts_parent_ms"] = [transit_parts(sect)], []
    for _ in range(args.alternate if args.parent_lib else 0):
        for lib, suffix in ((args.parent_lib, "_parent_ms"), (os.path.join(ROOT, "k-mer-count_amd", "libkmc.so"), "_ms")):
            _, s = run_child(args, kind, canonical, lib)
            maps, trs = base_times(s)
            row["map" + suffix].append(spread(maps))
            row["transits" + suffix].append(spread(trs))
            row["transits_parts" + suffix].append(transit_parts(s))
    assert row["variants_equal"], "the LDS-table and the plain form of the reduce pass disagree"
    if "host_equal" in row:
        assert row["host_equal"], "the host computation disagrees with the device: %s" % row["host_differs"]
        device = sum(row["pairs"][f]["median"] for f in passes[1:])
        row["host_over_device"] = (row["host_export_ms"] + row["host_numpy_ms"]) / device
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb-distinct", type=float, default=0.05, help="FASTA size of the all-distinct input")
    ap.add_argument("--genome", type=int, default=4_000_000, help="bases of the genome of the table with bubbles")
    ap.add_argument("--every", type=int, default=300, help="one substitution read per this many bases")
    ap.add_argument("--hot-reads", type=int, default=0, help="reads of the hot batch (0: as many as the table with bubbles has)")
    ap.add_argument("--bins", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tables", default="pool0,bubbles,hot")
    ap.add_argument("--forms", default="canonical,forward")
    ap.add_argument("--parent-lib", default="", help="a libkmc.so of the parent commit: its map and transits calls are timed in turn with this one's")
    ap.add_argument("--alternate", type=int, default=2, help="how often the two libraries take turns")
    ap.add_argument("--no-host", action="store_true", help="skip the numpy comparison")
    ap.add_argument("--base-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.child:
        child(args.child, args)
        return
    rows = []
    for kind in args.tables.split(","):
        for form in args.forms.split(","):
            row = measure(args, kind, form == "canonical")
            print(json.dumps(row), flush=True)
            rows.append(row)
            if args.out:
                with open(args.out, "w") as f:
                    json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
