#!/usr/bin/env python3
"""Time kmc_unitig_transits_device: the map passes it runs, the transit pass and the verdict pass, beside what
they are compared with.

Tables, k = 31, canonical and forward:
(a) pool0: synth pool 0 (every line fresh random: all-distinct; --gb-distinct 0.05 gives the 41.85 M-key tables of the other
    view rows), the counted batch walked through its own graph.  Few links: the floor.
(b) bubbles: the table with bubbles of tools/measure_simplify.py (4.41 M keys, 40 003 unitigs, 106 672 records with the
    defaults), walked by its own reads: real crossings.
(c) hot: the `repeat` input of tests/transit_inputs.py -- 44 reads over eight records and four slots -- repeated until the batch
    has as many reads as table (b)'s (--hot-reads to ask for more): every lane adds to the same few words.
Per table one child process with KMC_UNITIG_TRACE set, behind one warm call of each kind: --reps kmc_unitig_transits_device
calls (their trace lines give map_ms, transit_ms, verdict_ms), the same with KMC_TRANSITS_PLAIN set (every lane adds its own 1:
the A/B behind the per-wave combine; both must give the same arrays), --reps kmc_unitig_map_device calls on the same batch
(the yardstick: the parent's cost for the same segments) and --reps kmc_unitig_links_device calls.  On (b) and (c) the same
arrays are also made on the host from kmc_unitig_map + kmc_unitig_links with numpy, timed and compared word for word.  With
--parent-lib PATH (a libkmc.so of the parent commit) the map and links calls are also timed with that build, --alternate
times in turn with this one, each in a process of its own: they run no new code, so they have to stay inside the parent's own
run-to-run spread.  One JSON line per table on stdout, --out also writes them to a file."""
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

U64, I64 = np.uint64, np.int64
LINES = ("kmc_unitigs", "kmc_unitig_links", "kmc_unitig_map", "kmc_unitig_transits")


def host_transits(segs, seg_offsets, loffs, lto, min_reads):
    """(link_support, transit_offsets, transit_count, verdict, summary) from the host copies of a map result and the links,
    by the definitions of include/kmc.h, vectorised over the segments"""
    ns, nl, nu = len(segs), len(lto), (len(loffs) - 1) // 2
    loffs = loffs.astype(I64)
    to = np.concatenate([lto.astype(I64), np.full(4, -1, I64)])
    so = seg_offsets.astype(I64)
    start, ln, uni = segs[:, 0].astype(I64), segs[:, 1].astype(I64), segs[:, 2].astype(I64)
    first = np.zeros(ns + 1, bool)
    first[so[:-1][so[:-1] < so[1:]]] = True
    cross = np.zeros(ns + 1, bool)
    cross[1:ns] = ~first[1:ns] & (start[1:] == start[:-1] + ln[:-1])

    def rank(e, t):
        lo, d = loffs[e], loffs[e + 1] - loffs[e]
        r = np.full(len(e), 4, I64)
        for j in range(4):
            hit = (j < d) & (r == 4) & (to[np.minimum(lo + j, nl + 3)] == t)
            r[hit] = j
        return r, lo, d

    i = np.flatnonzero(cross[:ns])
    a, b = uni[i - 1] ^ 1, uni[i]
    r_ab, la, _ = rank(a, b)
    r_ba, lb, db = rank(b, a)
    sup = np.zeros(nl, U64)
    np.add.at(sup, (la + r_ab)[r_ab < 4], 1)
    np.add.at(sup, (lb + r_ba)[(r_ba < 4) & (a != b)], 1)
    orphan = int(((r_ab == 4) & (r_ba == 4)).sum())
    through = cross[i + 1]
    ti, p, dbt = i[through], r_ba[through], db[through]
    bb = uni[ti]
    q, _, d_out = rank(bb ^ 1, uni[np.minimum(ti + 1, ns - 1)] if ns else bb)
    ok = (p < 4) & (q < 4)
    o, v = bb & 1, bb >> 1
    P, Q, dE = np.where(o == 1, q, p), np.where(o == 1, p, q), np.where(o == 1, dbt, d_out)
    d_s, d_e = loffs[1::2] - loffs[0:-1:2], loffs[2::2] - loffs[1::2]
    toffs = np.concatenate([[0], np.cumsum(d_s * d_e)]).astype(I64)
    cnt = np.zeros(int(toffs[-1]), U64)
    np.add.at(cnt, (toffs[v] + P * dE + Q)[ok], 1)
    m = np.zeros((nu, 4, 4), bool)
    cpad = np.concatenate([cnt, np.zeros(16, U64)])
    for pp in range(4):
        for qq in range(4):
            valid = (pp < d_s) & (qq < d_e)
            m[:, pp, qq] = valid & (cpad[np.minimum(toffs[:-1] + pp * d_e + qq, len(cnt))] >= max(min_reads, 1))
    rows, cols = m.sum(2), m.sum(1)
    rng = np.arange(4)[None, :]
    repeat = (d_s >= 2) & (d_e >= 2)
    resolved = repeat & ((rows == 1) | (rng >= d_s[:, None])).all(1) & ((cols == 1) | (rng >= d_e[:, None])).all(1) & m.any((1, 2))
    verdict = np.where(~repeat, 0, np.where(~m.any((1, 2)), 1, np.where(resolved, 2, 3))).astype(np.uint8)
    summary = [len(i), orphan, int((sup == 0).sum()), int(ok.sum()), int((~ok).sum()), int(repeat.sum()), int((verdict == 2).sum()),
               int((verdict == 3).sum())]
    return sup, toffs.astype(U64), cnt, verdict, summary


def ev_ms(torch, stream, f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    f()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def bubble_read_count(args, k=31):
    return len(np.arange(0, args.genome - k, 1000 - (k - 1))) + len(np.arange(k, args.genome - k, args.every))


def child(spec, args):
    """one table: the calls whose trace lines the parent reads; everything else on stdout"""
    import torch
    kmc = importlib.import_module("k-mer-count_amd")
    kd = importlib.import_module("k-mer-count_amd.distributed")
    import measure_simplify
    kind, canonical = spec.split(",")[0], bool(int(spec.split(",")[1]))
    k, reps = 31, args.reps
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
        if kind == "pool0":
            s = kmc.Synth(seed=1, pool=0)
            n_reads, _ = kmc.synth_records_for_bytes(s, int(args.gb_distinct * 1e9))
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
            n_reads, n_bases = len(offs) - 1, len(bases)
            d_b, d_o = upload(bases, offs)
        else:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import map_inputs
            import transit_inputs
            sample, reads = transit_inputs.repeat(k, 500 + k)
            kc.add_batch(*map_inputs.pack(sample))
            one_b, one_o = map_inputs.pack(reads)
            copies = -(-(args.hot_reads or bubble_read_count(args)) // len(reads))
            bases = np.tile(one_b, copies)
            offs = np.concatenate([[0], (one_o[1:][None, :] + (np.arange(copies, dtype=U64) * U64(len(one_b)))[:, None]).ravel()]).astype(U64)
            n_reads, n_bases = len(offs) - 1, len(bases)
            d_b, d_o = upload(bases, offs)
            out["copies"] = copies
        torch.cuda.synchronize(dev)
        out["keys"] = kc.finalize()[0]
        batch = (d_b.data_ptr(), d_o.data_ptr(), n_reads, n_bases)
        os.environ.pop("KMC_TRANSITS_PLAIN", None)
        kc.unitig_links_device(1, 0)                 # warm: the buffers, the prefix index and the row index exist
        kc.map_reads_device(*batch, 1, 0)
        if not args.base_only:
            kc.transits_device(*batch, 1, 0)
            arrays = {}
            for name, plain in (("transits", False), ("plain", True)):
                if plain:
                    os.environ["KMC_TRANSITS_PLAIN"] = "1"
                mark("warm")
                kc.transits_device(*batch, 1, 0)
                mark(name)
                res = {}
                out[name + "_call_ms"] = [ev_ms(torch, stream, lambda: res.update(r=kc.transits_device(*batch, 1, 0))) for _ in range(reps)]
                ds, dt, dc, dv, nu, nl, nsl, summ = res["r"]
                words = lambda ptr, n: kd.device_view(ptr, max((n + 7) // 8, 1), dev).cpu().numpy().view(np.uint8)[:n].copy()
                arrays[name] = (words(ds, 8 * nl).view(U64), words(dt, 8 * (nu + 1)).view(U64), words(dc, 8 * nsl).view(U64), words(dv, nu))
                out.update(summary=summ.words(), unitigs=nu, records=nl, slots=nsl)
            os.environ.pop("KMC_TRANSITS_PLAIN", None)
            out["variants_equal"] = all(np.array_equal(x, y) for x, y in zip(arrays["transits"], arrays["plain"]))
        mark("map")
        out["map_call_ms"] = [ev_ms(torch, stream, lambda: kc.map_reads_device(*batch, 1, 0)) for _ in range(reps)]
        mark("links")
        out["links_call_ms"] = [ev_ms(torch, stream, lambda: kc.unitig_links_device(1, 0)) for _ in range(reps)]
        mark("end")
        out.update(reads=n_reads, bases=n_bases)
        if kind != "pool0" and not args.no_host and not args.base_only:
            os.environ.pop("KMC_UNITIG_TRACE", None)
            t0 = time.perf_counter()
            m, lk = kc.map_reads(bases, offs, 1, 0), kc.unitig_links(1, 0)
            t1 = time.perf_counter()
            host = host_transits(m.segments, m.seg_offsets, lk.offsets, lk.to, 1)
            t2 = time.perf_counter()
            out.update(host_export_ms=(t1 - t0) * 1e3, host_numpy_ms=(t2 - t1) * 1e3,
                       host_equal=bool(all(np.array_equal(x, y) for x, y in zip(host[:4], arrays["transits"])) and host[4] == out["summary"]))
        kc.close()
    print(json.dumps(out), flush=True)


def parse(line):
    return {name: float(val) if "." in val else int(val) for name, val in re.findall(r"(\w+) ([\d.]+)", line.split(":", 1)[1])}


def run_child(args, kind, canonical, lib=None):
    """(the child's JSON, {mark: its trace lines})"""
    env = dict(os.environ, KMC_UNITIG_TRACE="1")
    env.pop("KMC_TRANSITS_PLAIN", None)
    if lib:
        env["KMC_LIB_PATH"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", f"{kind},{int(canonical)}", "--gb-distinct", str(args.gb_distinct),
           "--genome", str(args.genome), "--every", str(args.every), "--reps", str(args.reps), "--hot-reads", str(args.hot_reads)]
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


def spread(ms):
    return dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)))


def base_times(sect):
    """(map: place_ms + segs_ms per call, links_ms per call) of a child's map and links sections"""
    maps = [parse(l) for l in sect["map"] if l.startswith("kmc_unitig_map:")]
    links = [parse(l) for l in sect["links"] if l.startswith("kmc_unitig_links:")]
    return [m["index_ms"] + m["place_ms"] + m["segs_ms"] for m in maps], [l["links_ms"] for l in links]


def measure(args, kind, canonical):
    res, sect = run_child(args, kind, canonical)
    row = dict(table=f"{kind}_k31_{'canonical' if canonical else 'forward'} ({res['keys']} keys)", **res)
    for name in ("transits", "plain"):
        lines = [parse(l) for l in sect[name] if l.startswith("kmc_unitig_transits:")]
        assert len(lines) == args.reps and all(l["links_reused"] == 1 for l in lines), sect[name]
        assert all(l.startswith("kmc_unitig_transits:") or l.startswith("kmc_unitig_map:") for l in sect[name]), "the unitigs and links were not reused"
        row[name] = {f: spread([l[f] for l in lines]) for f in ("map_ms", "transit_ms", "verdict_ms")}
    maps, links = base_times(sect)
    assert len(maps) == len(links) == args.reps
    row["map_ms"], row["links_ms"] = [spread(maps)], [spread(links)]
    row["transit_share_of_map"] = row["transits"]["transit_ms"]["median"] / row["map_ms"][0]["median"]
    row["plain_over_combined"] = row["plain"]["transit_ms"]["median"] / row["transits"]["transit_ms"]["median"]
    row["map_parent_ms"], row["links_parent_ms"] = [], []
    for _ in range(args.alternate if args.parent_lib else 0):
        for lib, suffix in ((args.parent_lib, "_parent_ms"), (os.path.join(ROOT, "k-mer-count_amd", "libkmc.so"), "_ms")):
            _, s = run_child(args, kind, canonical, lib)
            maps, links = base_times(s)
            row["map" + suffix].append(spread(maps))
            row["links" + suffix].append(spread(links))
    assert row["variants_equal"], "the combined and the plain form of the transit pass disagree"
    if "host_equal" in row:
        assert row["host_equal"], "the host computation disagrees with the device"
        row["host_over_device"] = (row["host_export_ms"] + row["host_numpy_ms"]) / (row["transits"]["transit_ms"]["median"] + row["transits"]["verdict_ms"]["median"])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb-distinct", type=float, default=0.05, help="FASTA size of the all-distinct input")
    ap.add_argument("--genome", type=int, default=4_000_000, help="bases of the genome of the table with bubbles")
    ap.add_argument("--every", type=int, default=300, help="one substitution read per this many bases")
    ap.add_argument("--hot-reads", type=int, default=0, help="reads of the hot-link batch (0: as many as the table with bubbles has)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tables", default="pool0,bubbles,hot")
    ap.add_argument("--forms", default="canonical,forward")
    ap.add_argument("--parent-lib", default="", help="a libkmc.so of the parent commit: its map and links calls are timed in turn with this one's")
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
