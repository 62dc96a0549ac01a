#!/usr/bin/env python3
"""Time kmc_unitig_contigs_device: the phases of its trace line, the ranking rounds, and the emit pass beside
what it is compared with.

Tables, k = 31, canonical:
(a) bubbles: the table with bubbles of tools/measure_transits.py (4.41 M keys with the defaults), walked by its own reads.
(b) pool0: synth pool 0 (all-distinct; --gb-distinct 0.05 gives the 41.85 M-key table of the other view rows), walked by its
    own reads.  Nothing is resolved there: the contigs are the unitigs and the emit pass copies them.
(c) chain: the `chain` input of tests/contig_inputs.py with --chain-repeats repeats in series: as many resolved repeats, two
    contigs of twice as many nodes and one.
Per table one child process with KMC_UNITIG_TRACE set.  Behind one transits call and one warm contigs call: --reps
kmc_unitig_contigs_device calls (their trace lines give choice_ms, rank_ms, layout_ms, emit_ms and the rounds), then in the same
process kmc_trim_device with KMC_TRIM_NONE on the contigs themselves -- a gather of as many bytes -- and kmc_read_peak_device
on a buffer of that size.  The emit pass's traffic is taken as bytes read + bytes written = 2 * bases.  Unless --no-host the
unitigs, links and transit arrays are copied out and the contigs are made on the host with numpy (host_contigs: the
definitions of include/kmc.h vectorised, pointer doubling over the node ends), timed and compared word for word.  With
--parent-lib PATH (a libkmc.so of the parent commit) kmc_unitigs_device, kmc_unitig_links_device and kmc_unitig_transits_device are timed with that
build and with this one in turn (--alternate), each in a process of its own: they run no new code, so they have to stay inside
the parent's own run-to-run spread.  One JSON line per table on stdout, --out also writes them to a file."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

U64, I64 = np.uint64, np.int64
PHASES = ("choice_ms", "rank_ms", "layout_ms", "emit_ms")


def host_contigs(loffs, lto, sup, toffs, tcnt, u_bases, u_offs, u_abund, k, min_reads, min_support):
    """(bases, offsets, path_offsets, path, abund, flags, summary) from the host copies of the unitigs, the links and the
    transit arrays, by the definitions of include/kmc.h, vectorised with numpy: pointer doubling over the node ends where
    tests/contig_model.py walks"""
    nl, nu = len(lto), (len(loffs) - 1) // 2
    z8 = np.zeros(0, np.uint8)
    if not nu:
        return z8, np.zeros(1, U64), np.zeros(1, U64), np.zeros(0, np.uint32), np.zeros(0, U64), z8, [0] * 8
    loffs, toffs, u_offs = loffs.astype(I64), toffs.astype(I64), u_offs.astype(I64)
    to = np.concatenate([lto.astype(I64), np.full(4, -1, I64)])
    spad = np.concatenate([sup.astype(U64), np.zeros(4, U64)])
    cpad = np.concatenate([tcnt.astype(U64), np.zeros(16, U64)])
    d_s, d_e = loffs[1::2] - loffs[0:-1:2], loffs[2::2] - loffs[1::2]
    m = np.zeros((nu, 4, 4), bool)
    for pp in range(4):
        for qq in range(4):
            m[:, pp, qq] = (pp < d_s) & (qq < d_e) & (cpad[np.minimum(toffs[:-1] + pp * d_e + qq, len(tcnt))] >= max(min_reads, 1))
    rows, cols, rng = m.sum(2), m.sum(1), np.arange(4)[None, :]
    resolved = (d_s >= 2) & (d_e >= 2) & ((rows == 1) | (rng >= d_s[:, None])).all(1) & ((cols == 1) | (rng >= d_e[:, None])).all(1)
    sigma, sigma_inv = m.argmax(2), m.argmax(1)                      # [u, P] -> Q, [u, Q] -> P
    copies = np.where(resolved, d_s, 1)
    node_off = np.concatenate([[0], np.cumsum(copies)])
    N = int(node_off[-1])
    owner = np.repeat(np.arange(nu), copies)
    cp = np.arange(N) - node_off[owner]
    ignored = 0
    if min_support:
        low = spad[:nl] < U64(min_support)
        end_of = np.repeat(np.arange(2 * nu), np.diff(loffs))
        ignored = int((low & ~resolved[end_of >> 1]).sum())
    # choice: a lane per node end in numpy
    a = np.arange(2 * N)
    n, e = a >> 1, (a & 1) ^ 1
    u, p = owner[n], cp[n]
    s = 2 * u + e
    lo, d = loffs[s], loffs[s + 1] - loffs[s]
    live = np.stack([(i < d) & ((min_support == 0) | (spad[np.minimum(lo + i, nl + 3)] >= U64(min_support))) for i in range(4)], 1)
    r = np.where(resolved[u], np.where(e == 0, p, sigma[u, np.minimum(p, 3)]), np.where(live.sum(1) == 1, live.argmax(1), -1))
    have = r >= 0
    t = to[np.where(have, lo + r, nl)]
    have &= t >= 0
    t = np.where(have, t, 0)
    w, f = t >> 1, t & 1
    lt, dt = loffs[t], loffs[t + 1] - loffs[t]
    back = np.stack([(i < dt) & (to[np.minimum(lt + i, nl + 3)] == s) for i in range(4)], 1)
    q = np.where(back.any(1), back.argmax(1), -1)
    copy = np.where(resolved[w], np.where(q < 0, -1, np.where(f == 0, q, sigma_inv[w, np.maximum(q, 0)])), 0)
    have &= copy >= 0
    link = np.where(have, 2 * (node_off[w] + copy) + (f == 0), -1)
    joined = np.where((link >= 0) & (link != a) & (link[np.maximum(link, 0)] == a), link, -1)

    def rank(joined):
        ptr, dist = np.where(joined >= 0, joined ^ 1, a), (joined >= 0).astype(I64)
        for _ in range(max(1, int(2 * N - 1).bit_length()) + 1):
            ptr, dist = ptr[ptr], dist + dist[ptr]
        return ptr, dist

    ptr, dist = rank(joined)
    circ = np.zeros(N, bool)
    on_cycle = joined[ptr] >= 0
    if on_cycle.any():
        nxt, mn = np.where(joined >= 0, joined ^ 1, a), n.copy()
        for _ in range(max(1, int(2 * N - 1).bit_length())):
            mn, nxt = np.minimum(mn, mn[nxt]), nxt[nxt]
        cut = np.flatnonzero(on_cycle[1::2] & (mn[1::2] == np.arange(N)))      # nodes that are their cycle's smallest
        partner = joined[2 * cut + 1]
        joined[partner] = -1
        joined[2 * cut + 1] = -1
        circ[cut] = True
        ptr, dist = rank(joined)
    # layout
    er, el, dx, dy = ptr[0::2] >> 1, ptr[1::2] >> 1, dist[0::2], dist[1::2]
    rc = er < el
    first, pos, ln = np.where(rc, er, el), np.where(rc, dx, dy), dx + dy + 1
    is_first = pos == 0
    nc = int(is_first.sum())
    cid_of = np.cumsum(is_first) - is_first
    poff_of = np.cumsum(np.where(is_first, ln, 0)) - np.where(is_first, ln, 0)
    slot, cid = poff_of[first] + pos, cid_of[first]
    path = np.zeros(N, np.uint32)
    path[slot] = (2 * owner + rc).astype(np.uint32)
    starts = np.flatnonzero(is_first)
    path_offsets = np.concatenate([poff_of[starts], [N]]).astype(U64)
    flags = circ[starts].astype(np.uint8)
    abund = np.zeros(nc, U64)
    np.add.at(abund, cid, u_abund[owner].astype(U64))
    # spelling: slot by slot, every output base's source index
    pu, po = path.astype(I64) >> 1, path.astype(I64) & 1
    ulen = u_offs[pu + 1] - u_offs[pu]
    head = np.zeros(N, bool)
    head[path_offsets[:-1].astype(I64)] = True
    skip = np.where(head, 0, k - 1)
    slen = ulen - skip
    sstart = np.concatenate([[0], np.cumsum(slen)])
    src0 = np.where(po == 1, u_offs[pu] + ulen - 1 - skip, u_offs[pu] + skip)
    j = np.repeat(np.arange(N), slen)
    o = np.arange(int(sstart[-1])) - sstart[j]
    rev = po[j] == 1
    raw = u_bases[np.where(rev, src0[j] - o, src0[j] + o)]
    comp = np.arange(256, dtype=np.uint8)
    comp[[65, 67, 71, 84]] = [84, 71, 67, 65]
    bases = np.where(rev, comp[raw], raw).astype(np.uint8)
    offsets = sstart[np.concatenate([path_offsets[:-1].astype(I64), [N]])].astype(U64)
    sizes = np.diff(path_offsets.astype(I64))
    summary = [nc, N, int(resolved.sum()), ignored, int(flags.sum()), int((sizes == 1).sum()), int(sizes.max()), int(sstart[-1])]
    return bases, offsets, path_offsets, path, abund, flags, summary


def ev_ms(torch, stream, f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    f()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def child(spec, args):
    import torch
    kmc = importlib.import_module("k-mer-count_amd")
    kd = importlib.import_module("k-mer-count_amd.distributed")
    import measure_simplify
    k, reps, canonical = 31, args.reps, True
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
        if spec == "pool0":
            s = kmc.Synth(seed=1, pool=0)
            n_reads, _ = kmc.synth_records_for_bytes(s, int(args.gb_distinct * 1e9))
            n_bases = n_reads * s.read_len
            d_b = torch.zeros(n_bases + 64, dtype=torch.uint8, device=dev)
            d_o = torch.empty(n_reads + 1, dtype=torch.int64, device=dev)
            kmc.synth_reads_device(s, 0, n_reads, d_b.data_ptr(), d_o.data_ptr(), 0, stream.cuda_stream)
            stream.synchronize()
            kc.add_batch_device(d_b.data_ptr(), d_o.data_ptr(), n_reads, n_bases, s.read_len)
        elif spec == "bubbles":
            (gb_, go), (sb, so), _ = measure_simplify.bubble_reads(args.genome, args.every, k, 1)
            for _ in range(3):
                kc.add_batch(gb_, go)
            kc.add_batch(sb, so)
            bases, offs = np.concatenate([gb_, sb]), np.concatenate([go, so[1:] + go[-1]]).astype(U64)
            n_reads, n_bases = len(offs) - 1, len(bases)
            d_b, d_o = upload(bases, offs)
        else:
            import contig_inputs
            import map_inputs
            case = contig_inputs.chain(k, 1, repeats=args.chain_repeats)
            kc.add_batch(*map_inputs.pack(case.sample))
            bases, offs = map_inputs.pack(case.reads)
            n_reads, n_bases = len(offs) - 1, len(bases)
            d_b, d_o = upload(bases, offs)
        torch.cuda.synchronize(dev)
        out["keys"] = kc.finalize()[0]
        batch = (d_b.data_ptr(), d_o.data_ptr(), n_reads, n_bases)
        mark("base")
        out["unitigs_call_ms"] = [ev_ms(torch, stream, lambda: kc.unitigs_device(1, 0)) for _ in range(reps)]
        out["links_call_ms"] = [ev_ms(torch, stream, lambda: kc.unitig_links_device(1, 0)) for _ in range(reps)]
        out["transits_call_ms"] = [ev_ms(torch, stream, lambda: kc.transits_device(*batch, 1, 0)) for _ in range(reps)]
        if not args.base_only:
            kc.contigs_device(1, 0, 1, args.min_support)
            mark("contigs")
            res = {}
            out["contigs_call_ms"] = [ev_ms(torch, stream, lambda: res.update(r=kc.contigs_device(1, 0, 1, args.min_support))) for _ in range(reps)]
            db, do, dp, dn, da, df, nc, nn, nb, summ = res["r"]
            out.update(summary=summ.words(), contigs=nc, nodes=nn, bases=nb)
            mark("trim")
            kc.trim_reads_device(db, do, nc, nb, 1, 0, kmc.TRIM_NONE)
            out["trim_call_ms"] = [ev_ms(torch, stream, lambda: kc.trim_reads_device(db, do, nc, nb, 1, 0, kmc.TRIM_NONE)) for _ in range(reps)]
            mark("end")
            d_e = torch.zeros(nb // 16 * 16 + 64, dtype=torch.uint8, device=dev)
            peak_ms, _ = kmc.read_peak_device(d_e.data_ptr(), nb // 16 * 16, 0, stream.cuda_stream)
            out["read_peak_bytes_per_s"] = (nb // 16 * 16) / (peak_ms * 1e-3)
            if not args.no_host:
                os.environ.pop("KMC_UNITIG_TRACE", None)
                words = lambda ptr, n: kd.device_view(ptr, max((n + 7) // 8, 1), dev).cpu().numpy().view(np.uint8)[:n].copy()
                got = (words(db, nb), words(do, 8 * (nc + 1)).view(U64), words(dp, 8 * (nc + 1)).view(U64), words(dn, 4 * nn).view(np.uint32),
                       words(da, 8 * nc).view(U64), words(df, nc))
                t0 = time.perf_counter()
                tr = kc.transits(np.zeros(0, np.uint8), np.zeros(1, U64), 1, 0, accumulate=True)       # the held totals, copied out
                u = kc.unitigs(1, 0)
                t1 = time.perf_counter()
                host = host_contigs(tr.links.offsets, tr.links.to, tr.link_support, tr.transit_offsets, tr.transit_count, u.bases, u.offsets, u.abund, k, 1,
                                    args.min_support)
                t2 = time.perf_counter()
                out.update(host_export_ms=(t1 - t0) * 1e3, host_numpy_ms=(t2 - t1) * 1e3,
                           host_equal=bool(all(np.array_equal(x, y) for x, y in zip(got, host[:6])) and host[6] == out["summary"]))
        out.update(reads=n_reads, read_bases=n_bases)
        kc.close()
    print(json.dumps(out), flush=True)


def parse(line):
    return {name: float(val) if "." in val else int(val) for name, val in re.findall(r"(\w+) ([\d.]+)", line.split(":", 1)[1])}


def run_child(args, kind, lib=None):
    """(the child's JSON, {mark: its trace lines})"""
    env = dict(os.environ, KMC_UNITIG_TRACE="1")
    if lib:
        env["KMC_LIB_PATH"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--gb-distinct", str(args.gb_distinct), "--genome", str(args.genome),
           "--every", str(args.every), "--reps", str(args.reps), "--chain-repeats", str(args.chain_repeats), "--min-support", str(args.min_support)]
    cmd += (["--no-host"] if args.no_host else []) + (["--base-only"] if lib else [])
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    if r.returncode:                            # nothing more is started on a device where a process has just failed
        raise RuntimeError("the traced child failed (exit %d): %s" % (r.returncode, r.stderr[-600:]))
    sect, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("mark "):
            cur = line[5:]
            sect[cur] = []
        elif cur and line.startswith("kmc_"):
            sect[cur].append(line)
    return json.loads(r.stdout.strip().splitlines()[-1]), sect


def spread(ms):
    return dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)))


def measure(args, kind):
    res, sect = run_child(args, kind)
    row = dict(table=f"{kind}_k31_canonical ({res['keys']} keys)", **res)
    lines = [parse(l) for l in sect["contigs"] if l.startswith("kmc_unitig_contigs:")]
    assert len(lines) == args.reps and len(sect["contigs"]) == args.reps, sect["contigs"]       # nothing but the contigs pass computed
    row["phases"] = {f: spread([l[f] for l in lines]) for f in PHASES}
    row["rounds"] = lines[0]["rounds"]
    row["emit_bytes_per_s"] = 2.0 * res["bases"] / (row["phases"]["emit_ms"]["median"] * 1e-3)
    trims = [parse(l) for l in sect["trim"] if l.startswith("kmc_trim:")][-args.reps:]
    row["trim_gather_ms"] = spread([t["gather_ms"] for t in trims])
    row["trim_gather_bytes_per_s"] = 2.0 * res["bases"] / (row["trim_gather_ms"]["median"] * 1e-3)
    row["emit_of_trim_gather"] = row["emit_bytes_per_s"] / row["trim_gather_bytes_per_s"]
    row["emit_of_read_peak"] = row["emit_bytes_per_s"] / res["read_peak_bytes_per_s"]
    for name in ("unitigs", "links", "transits", "contigs", "trim"):
        row[name + "_call_ms"] = [spread(res[name + "_call_ms"])]
    for name in ("unitigs", "links", "transits"):
        row[name + "_parent_call_ms"] = []
    for _ in range(args.alternate if args.parent_lib else 0):
        for lib, suffix in ((args.parent_lib, "_parent_call_ms"), (os.path.join(ROOT, "k-mer-count_amd", "libkmc.so"), "_call_ms")):
            r, _ = run_child(args, kind, lib)
            for name in ("unitigs", "links", "transits"):
                row[name + suffix].append(spread(r[name + "_call_ms"]))
    if "host_equal" in row:
        assert row["host_equal"], "the host computation disagrees with the device"
        row["host_over_device"] = (row["host_export_ms"] + row["host_numpy_ms"]) / sum(row["phases"][f]["median"] for f in PHASES)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb-distinct", type=float, default=0.05, help="FASTA size of the all-distinct input")
    ap.add_argument("--genome", type=int, default=4_000_000, help="bases of the genome of the table with bubbles")
    ap.add_argument("--every", type=int, default=300, help="one substitution read per this many bases")
    ap.add_argument("--chain-repeats", type=int, default=20000, help="repeats in series of the chain table")
    ap.add_argument("--min-support", type=int, default=0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tables", default="bubbles,pool0,chain")
    ap.add_argument("--parent-lib", default="", help="a libkmc.so of the parent commit: its unitigs, links and transits calls are timed in turn with this one's")
    ap.add_argument("--alternate", type=int, default=2, help="how often the two libraries take turns")
    ap.add_argument("--no-host", action="store_true", help="skip the host comparison")
    ap.add_argument("--base-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.child:
        child(args.child, args)
        return
    rows = []
    for kind in args.tables.split(","):
        row = measure(args, kind)
        print(json.dumps(row), flush=True)
        rows.append(row)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
