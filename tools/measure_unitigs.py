#!/usr/bin/env python3
"""Time kmc_unitigs_device on the views real finalizes leave, beside the same answer obtained with what the
library offered before it.

Tables: those of tools/measure_graph.py -- synth pool 0 (every line fresh random: all-distinct, the sort path) and the
benchmark's pool-10 generator input (a few thousand keys), k = 31, --gb GB of FASTA each, canonical and forward.  Per table
and range:
  * kmc_unitigs_device: event pairs on the ctx's stream around whole calls, --warmup untimed, --reps timed, median and
    minimum;
  * its phases (adj, links, ranking and the number of rounds, cycles, layout, emit): one more call in a child process with
    KMC_UNITIG_TRACE set, which makes the library print its own event times;
  * the comparator, a thing of this tool only and not product code: kmc_graph and kmc_export to the host, then the walk
    DESIGN §4.10 describes, with numpy where it vectorises -- neighbour keys by shifts and masks, their rows by
    searchsorted, the mutual join, pointer jumping over the side states, cycles cut at their smallest row, then the
    spelling.  Wall-clock time, copies included: a user pays them.  Its result must equal the kernel's, array for array.
One JSON line per measurement on stdout; --out also writes them all to a file."""
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
import torch  # noqa: E402

kmc = importlib.import_module("k-mer-count_amd")
kd = importlib.import_module("k-mer-count_amd.distributed")
U64, U32 = np.uint64, np.uint32
NONE = np.uint32(0xFFFFFFFF)


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


def revcomp_u64(x, k):
    """reverse complement of one-word keys (uint64 array, k <= 32)"""
    y = ~x
    for s, m in ((2, 0x3333333333333333), (4, 0x0F0F0F0F0F0F0F0F), (8, 0x00FF00FF00FF00FF), (16, 0x0000FFFF0000FFFF),
                 (32, 0x00000000FFFFFFFF)):
        y = ((y >> U64(s)) & U64(m)) | ((y & U64(m)) << U64(s))
    return y >> U64(64 - 2 * k)


def _rank(joined):
    """(end state, distance) of every side state by pointer jumping; states on cycles keep a joined pointer"""
    n2 = len(joined)
    a = np.arange(n2, dtype=U32)
    term = joined == NONE
    ptr = np.where(term, a, joined ^ U32(1))
    dist = np.where(term, 0, 1).astype(U32)
    for _ in range(max(1, int(n2).bit_length()) + 1):
        nxt = ptr[ptr]
        if np.array_equal(nxt, ptr):
            break
        dist = dist + dist[ptr]
        ptr = nxt
    return ptr, dist


def host_unitigs(keys, cnt, adj, k, canonical):
    """(bases, offsets, abund, flags, words) from the exported view and the adj words of kmc_graph"""
    n = len(keys)
    mask, tb = U64((1 << (2 * k)) - 1), U64(2 * k - 2)
    ctz = np.array([0, 0, 1, 0, 2, 0, 1, 0, 3, 0, 1, 0, 2, 0, 1, 0], U64)
    solid = (adj >> 10) & 1 == 1
    link = np.full(2 * n, NONE, U32)
    for side in (0, 1):
        go = np.nonzero(solid & ((adj >> (8 + side)) & 1 == 0))[0]
        x = keys[go]
        c = ctz[(adj[go] >> (4 * side)) & 15]
        f = ((x << U64(2)) & mask) | c if side == 0 else (x >> U64(2)) | (c << tb)
        kept_face = 1 - side                       # kept as it is: entered on the opposite side
        face = np.full(len(go), kept_face, U32)
        if canonical:
            q = revcomp_u64(f, k)
            face = np.where(q < f, U32(side), U32(kept_face))
            f = np.minimum(f, q)
        row = np.searchsorted(keys, f).astype(U32)
        link[2 * go + side] = 2 * row + face
    a = np.arange(2 * n, dtype=U32)
    has = link != NONE
    back = np.where(has, link[np.where(has, link, 0)], NONE)
    ok = has & (link != a) & (back == a)
    joined = np.where(ok, link, NONE)
    lost = int(has.sum() - ok.sum())
    ptr, dist = _rank(joined)
    circ = np.zeros(n, bool)
    cyc = joined[ptr] != NONE
    if cyc.any():
        mrow, p = (a >> U32(1)), np.where(joined == NONE, a, joined ^ U32(1))
        for _ in range(int(cyc.sum()).bit_length()):
            mrow, p = np.minimum(mrow, mrow[p]), p[p]
        rows = np.nonzero(cyc[1::2] & (mrow[1::2] == np.arange(n, dtype=U32)))[0]
        cut = (2 * rows + 1).astype(U32)
        other = joined[cut]
        joined[cut] = NONE
        joined[other] = NONE
        circ[rows] = True
        ptr, dist = _rank(joined)
    er, el, dr, dl = ptr[0::2] >> U32(1), ptr[1::2] >> U32(1), dist[0::2], dist[1::2]
    rc = (er < el) if canonical else np.zeros(n, bool)
    first, pos, ln = np.where(rc, er, el), np.where(rc, dr, dl), dr + dl + 1
    isf = solid & (pos == 0)
    uid_at = np.cumsum(isf) - isf
    koff_at = np.cumsum(np.where(isf, ln, 0).astype(np.int64)) - np.where(isf, ln, 0)
    s = np.nonzero(solid)[0]
    uid, at = uid_at[first[s]], koff_at[first[s]] + uid_at[first[s]] * (k - 1)
    nu, nk = int(isf.sum()), len(s)
    nb = nk + (k - 1) * nu
    bases = np.zeros(nb, np.uint8)
    ascii_ = np.frombuffer(b"ACGT", np.uint8)
    top = (keys[s] >> tb) & U64(3)
    last = np.where(rc[s], U64(3) - top, keys[s] & U64(3))
    bases[at + (k - 1) + pos[s]] = ascii_[last]
    fs = np.nonzero(isf)[0]
    fk = np.where(rc[fs], revcomp_u64(keys[fs], k), keys[fs])
    fat = koff_at[fs] + uid_at[fs] * (k - 1)
    for j in range(k):
        bases[fat + j] = ascii_[(fk >> U64(2 * (k - 1 - j))) & U64(3)]
    offsets = np.concatenate([fat, [nb]]).astype(U64)
    abund = np.zeros(nu, U64)
    np.add.at(abund, uid, cnt[s])
    flags = circ[fs].astype(np.uint8)
    words = [nu, nb, nk, int(flags.sum()), int((ln[fs] == 1).sum()), int(ln[fs].max()) if nu else 0, lost, int(abund.sum())]
    return bases, offsets, abund, flags, words


def comparator(kc, k, canonical, lo_c, hi_c):
    t = kc.export()
    adj, _ = kc.graph(lo_c, hi_c)
    return host_unitigs(t.key_lo, t.count, adj, k, canonical)


def dev_array(ptr, n_bytes, dev):
    if not n_bytes:
        return np.zeros(0, np.uint8)
    return kd.device_view(ptr, (n_bytes + 7) // 8, dev).cpu().numpy().view(np.uint8)[:n_bytes]


def make_ctx(args, pool, canonical, k, stream, dev):
    s = kmc.Synth(seed=1, pool=pool)
    n_rec, _ = kmc.synth_records_for_bytes(s, int(args.gb * 1e9))
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


def trace_child(args, pool, canonical, k, lo_c, hi_c):
    """the library's own phase times of one warm call: {phase_ms..., rounds, cycle_states}"""
    env = dict(os.environ, KMC_UNITIG_TRACE="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--trace-one", f"{pool},{int(canonical)},{k},{lo_c},{hi_c}",
                        "--gb", str(args.gb)], capture_output=True, text=True, env=env)
    lines = [l for l in r.stderr.splitlines() if l.startswith("kmc_unitigs:")]
    if r.returncode or not lines:          # nothing more is started on a device where a process has just failed
        raise RuntimeError("the traced call failed (exit %d): %s" % (r.returncode, r.stderr[-300:]))
    out = {}
    for name, val in re.findall(r"(\w+) ([\d.]+)", lines[-1]):
        out[name] = float(val) if "." in val else int(val)
    return out


def measure(args, pool, canonical, k=31):
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        kc, nd = make_ctx(args, pool, canonical, k, stream, dev)
        name = f"pool{pool}_k{k}_{'canonical' if canonical else 'forward'} ({args.gb:g} GB, {nd} keys)"
        for lo_c, hi_c in ((1, 0), (2, 0)):
            res = {}
            med, mn = ev_timed(stream, lambda: res.update(u=kc.unitigs_device(lo_c, hi_c)), args.warmup, args.reps)
            db, do, da, df, nu, nb, summ = res["u"]
            got = (dev_array(db, nb, dev).copy(), dev_array(do, 8 * (nu + 1), dev).view(U64).copy(), dev_array(da, 8 * nu, dev).view(U64).copy(),
                   dev_array(df, nu, dev).copy())
            ctimes = []
            for _ in range(args.comparator_reps):
                t0 = time.perf_counter()
                want = comparator(kc, k, canonical, lo_c, hi_c)
                ctimes.append((time.perf_counter() - t0) * 1e3)
            same = all(np.array_equal(g, w) for g, w in zip(got, want[:4])) and want[4] == summ.words()
            cmed = float(np.median(ctimes))
            row = dict(table=name, call="kmc_unitigs_device", range=[lo_c, hi_c], n=nd, summary=summ.words(), ms_median=med, ms_min=mn,
                            comparator_ms_median=cmed, comparator_ms_min=float(min(ctimes)), ratio_comparator_over_unitigs=cmed / med,
                            phases=trace_child(args, pool, canonical, k, lo_c, hi_c), comparator_equal=same)
            assert same, "the comparator and kmc_unitigs_device disagree"
            yield row
        kc.close()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--comparator-reps", type=int, default=1)
    ap.add_argument("--pools", default="0,10")
    ap.add_argument("--small", action="store_true", help="a quick pass: 0.05 GB")
    ap.add_argument("--trace-one", default="", help=argparse.SUPPRESS)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.small:
        args.gb = 0.05
    if args.trace_one:
        pool, canonical, k, lo_c, hi_c = [int(x) for x in args.trace_one.split(",")]
        dev = torch.device("cuda", 0)
        stream = torch.cuda.Stream(dev)
        with torch.cuda.stream(stream):
            kc, _ = make_ctx(args, pool, bool(canonical), k, stream, dev)
            os.environ.pop("KMC_UNITIG_TRACE")
            kc.unitigs_device(lo_c, hi_c)          # warm: buffers and the index exist
            os.environ["KMC_UNITIG_TRACE"] = "1"
            kc.unitigs_device(lo_c, hi_c)
            kc.close()
        return
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
