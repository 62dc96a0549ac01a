#!/usr/bin/env python3
"""Time kmc_unitig_map_device: the row index, the place pass and the segment passes, beside what they are
compared with.

Tables, k = 31, canonical and forward: synth pool 0 (every line fresh random: all-distinct, --gb-distinct GB of FASTA) and,
with --pools, the generator's other pools.  The batch that is mapped is the batch that was counted.  Per table, in a child
process with KMC_UNITIG_TRACE set so that the library prints its own event times:
  * one kmc_unitigs_device call (its phases, for the comparison with the parent commit) and one kmc_unitig_clean_device
    call behind it (clean_ms): neither runs new code;
  * the first map call behind a unitig result (index_ms: the row index is built) and --reps more (index_ms ~ 0, place_ms,
    segs_ms, median and minimum), windows per second from place_ms + segs_ms;
  * the same with KMC_MAP_NO_INDEX set: the place kernel built to gather adj, the ranking and uid_of per window -- the A/B
    behind the index; both variants must give the same arrays;
  * kmc_profile_device on the same batch and view, timed with event pairs on the ctx's stream: the same windows with a
    count lookup, the floor of the place pass;
  * with --host-model (k <= 31): the same place words from kmc_unitigs and numpy on the host (sort the unitigs' keys,
    search every window), timed with the wall clock.
One JSON line per table on stdout; --out also writes them to a file."""
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


def _keys(codes, valid, k):
    """(forward key, reverse-complement key, valid) of the window starting at every position of a code array (k <= 31)"""
    n = len(codes)
    fw, rc = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    ok = np.ones(n, bool)
    for i in range(k):
        c = np.zeros(n, np.uint64)
        c[:n - i] = codes[i:]
        v = np.zeros(n, bool)
        v[:n - i] = valid[i:]
        fw = (fw << np.uint64(2)) | c
        rc |= (np.uint64(3) - c) << np.uint64(2 * i)
        ok &= v
    return fw, rc, ok


def host_place(kc, bases, offs, k, canonical, lo_c, hi_c):
    """the place words from kmc_unitigs and numpy: every key of every unitig with (unitig, position), sorted; every window
    of the batch searched in them"""
    lut = np.full(256, 4, np.uint8)
    lut[[65, 67, 71, 84]] = [0, 1, 2, 3]
    u = kc.unitigs(lo_c, hi_c)
    ucodes = lut[u.bases].astype(np.uint64)
    fw, rc, _ = _keys(ucodes, np.ones(len(ucodes), bool), k)
    uo = u.offsets.astype(np.int64)
    uid = np.searchsorted(uo, np.arange(len(ucodes)), side="right") - 1
    pos = np.arange(len(ucodes)) - uo[uid]
    is_key = pos + k <= (uo[uid + 1] - uo[uid]) if len(uid) else np.zeros(0, bool)
    key = np.minimum(fw, rc) if canonical else fw
    key, uid, pos, stored_rc = key[is_key], uid[is_key], pos[is_key], (rc < fw)[is_key] if canonical else np.zeros(int(is_key.sum()), bool)
    order = np.argsort(key, kind="stable")
    key, uid, pos, stored_rc = key[order], uid[order], pos[order], stored_rc[order]
    codes = lut[bases]
    valid = codes < 4
    starts = np.zeros(len(bases) + 1, np.int64)
    np.add.at(starts, offs.astype(np.int64), 1)
    rid = np.cumsum(starts[:len(bases)]) - 1
    wf, wr, ok = _keys(np.where(valid, codes, 0).astype(np.uint64), valid, k)
    ok &= np.arange(len(bases)) + k <= offs.astype(np.int64)[rid + 1]
    wk = np.minimum(wf, wr) if canonical else wf
    at = np.minimum(np.searchsorted(key, wk), max(len(key) - 1, 0))
    hit = ok & (key[at] == wk) if len(key) else np.zeros(len(bases), bool)
    flipped = (wr < wf) if canonical else np.zeros(len(bases), bool)
    o = (flipped ^ stored_rc[at]) & (wr != wf)
    place = np.full(len(bases), 0xFFFFFFFF, np.uint64)
    place[hit] = (pos[at][hit].astype(np.uint64) << np.uint64(32)) | (uid[at][hit].astype(np.uint64) * np.uint64(2) + o[hit].astype(np.uint64))
    return place


def child(spec, gb, reps, host_model):
    pool, canonical, k, lo_c, hi_c = [int(x) for x in spec.split(",")]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    out = {}
    with torch.cuda.stream(stream):
        s = kmc.Synth(seed=1, pool=pool)
        n_rec, _ = kmc.synth_records_for_bytes(s, int(gb * 1e9))
        n_bases = n_rec * s.read_len
        d_b = torch.zeros(n_bases + 64, dtype=torch.uint8, device=dev)
        d_o = torch.empty(n_rec + 1, dtype=torch.int64, device=dev)
        kmc.synth_reads_device(s, 0, n_rec, d_b.data_ptr(), d_o.data_ptr(), 0, stream.cuda_stream)
        stream.synchronize()
        kc = kmc.KmerCounter(k=k, canonical=bool(canonical), stream=stream.cuda_stream)
        kc.add_batch_device(d_b.data_ptr(), d_o.data_ptr(), n_rec, n_bases, s.read_len)
        nd, _ = kc.finalize()
        batch = (d_b.data_ptr(), d_o.data_ptr(), n_rec, n_bases)
        os.environ.pop("KMC_UNITIG_TRACE", None)
        os.environ.pop("KMC_MAP_NO_INDEX", None)
        kc.unitigs_device(lo_c, hi_c)              # warm: buffers and the prefix index exist
        kc.map_reads_device(*batch, lo_c, hi_c)
        kc.clean_unitigs_device(lo_c, hi_c)
        d_win = torch.zeros(n_bases, dtype=torch.int32, device=dev)
        d_st = torch.zeros((n_rec, kmc.PROFILE_WORDS), dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        prof = lambda: kc.profile_device(batch[0], batch[1], n_rec, n_bases, 1, d_win.data_ptr(), d_st.data_ptr())
        prof()
        out["profile_ms"] = [ev_ms(stream, prof) for _ in range(reps)]
        os.environ["KMC_UNITIG_TRACE"] = "1"
        print("mark unitigs", file=sys.stderr, flush=True)
        kc.unitigs_device(lo_c, hi_c)
        print("mark first", file=sys.stderr, flush=True)
        kc.map_reads_device(*batch, lo_c, hi_c)    # behind a fresh unitig result: builds the row index
        arrays = {}
        for name, no_index in (("index", False), ("three_gathers", True)):
            if no_index:
                os.environ["KMC_MAP_NO_INDEX"] = "1"
            else:
                os.environ.pop("KMC_MAP_NO_INDEX", None)
            print("mark warm", file=sys.stderr, flush=True)
            kc.map_reads_device(*batch, lo_c, hi_c)
            print("mark " + name, file=sys.stderr, flush=True)
            res = {}
            ms = [ev_ms(stream, lambda: res.update(r=kc.map_reads_device(*batch, lo_c, hi_c))) for _ in range(reps)]
            dp, ds, dso, dg, du, ns, nu, summ = res["r"]
            arrays[name] = (dev_words(dp, 8 * n_bases, dev), dev_words(ds, 16 * n_rec, dev), dev_words(dso, 8 * (n_rec + 1), dev),
                            dev_words(dg, 16 * ns, dev), dev_words(du, 8 * nu, dev))
            out[name + "_call_ms"] = ms
            out["summary"] = summ.words()
        os.environ.pop("KMC_MAP_NO_INDEX", None)
        print("mark clean", file=sys.stderr, flush=True)
        kc.clean_unitigs_device(lo_c, hi_c)
        print("mark end", file=sys.stderr, flush=True)
        os.environ.pop("KMC_UNITIG_TRACE", None)
        out["variants_equal"] = all(np.array_equal(a, b) for a, b in zip(arrays["index"], arrays["three_gathers"]))
        out["keys"], out["reads"], out["bases"] = nd, n_rec, n_bases
        if host_model and k <= 31:
            hb, ho = d_b[:n_bases].cpu().numpy(), d_o.cpu().numpy().astype(np.uint64)
            t0 = time.perf_counter()
            want = host_place(kc, hb, ho, k, bool(canonical), lo_c, hi_c)
            out["host_model_s"] = time.perf_counter() - t0
            out["host_model_equal"] = bool(np.array_equal(want, arrays["index"][0].view(np.uint64)))
        kc.close()
    print(json.dumps(out), flush=True)


def parse(line):
    return {name: float(val) if "." in val else int(val) for name, val in re.findall(r"(\w+) ([\d.]+)", line.split(":", 1)[1])}


def measure(args, pool, canonical, gb, lo_c, hi_c, k=31):
    env = dict(os.environ, KMC_UNITIG_TRACE="1")
    env.pop("KMC_MAP_NO_INDEX", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", f"{pool},{int(canonical)},{k},{lo_c},{hi_c}", "--gb", str(gb), "--reps", str(args.reps)]
    r = subprocess.run(cmd + (["--host-model"] if args.host_model else []), capture_output=True, text=True, env=env)
    if r.returncode:                            # nothing more is started on a device where a process has just failed
        raise RuntimeError("the traced child failed (exit %d): %s" % (r.returncode, r.stderr[-600:]))
    res = json.loads(r.stdout.strip().splitlines()[-1])
    sect, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("mark "):
            cur = line[5:]
            sect[cur] = []
        elif cur and line.startswith("kmc_unitig"):
            sect[cur].append(line)
    phases = parse([l for l in sect["unitigs"] if l.startswith("kmc_unitigs:")][-1])
    first = parse([l for l in sect["first"] if l.startswith("kmc_unitig_map:")][-1])
    clean = [parse(l) for l in sect["clean"] if l.startswith("kmc_unitig_clean:")]
    row = dict(table=f"pool{pool}_k{k}_{'canonical' if canonical else 'forward'} ({gb:g} GB, {res['keys']} keys)", range=[lo_c, hi_c],
               keys=res["keys"], reads=res["reads"], bases=res["bases"], summary=res["summary"], unitigs_phases=phases,
               unitigs_ms=sum(v for n, v in phases.items() if n.endswith("_ms")), clean_ms=clean[-1]["clean_ms"] if clean else None,
               index_ms=first["index_ms"], first_call=first, profile_ms_median=float(np.median(res["profile_ms"])),
               profile_ms_min=float(min(res["profile_ms"])), variants_equal=res["variants_equal"])
    for name in ("index", "three_gathers"):
        lines = [parse(l) for l in sect[name] if l.startswith("kmc_unitig_map:")]
        assert len(lines) == args.reps and all(l["unitigs_reused"] == 1 for l in lines), sect[name]
        place, segs = [l["place_ms"] for l in lines], [l["segs_ms"] for l in lines]
        row[name] = dict(place_ms_median=float(np.median(place)), place_ms_min=float(min(place)), segs_ms_median=float(np.median(segs)),
                         segs_ms_min=float(min(segs)), index_ms_median=float(np.median([l["index_ms"] for l in lines])),
                         call_ms_median=float(np.median(res[name + "_call_ms"])), call_ms_min=float(min(res[name + "_call_ms"])))
    windows = res["summary"][1]
    row["windows_per_s"] = windows / ((row["index"]["place_ms_median"] + row["index"]["segs_ms_median"]) * 1e-3)
    row["place_over_profile"] = row["index"]["place_ms_median"] / row["profile_ms_median"]
    row["three_gathers_over_index"] = row["three_gathers"]["place_ms_median"] / row["index"]["place_ms_median"]
    for name in ("host_model_s", "host_model_equal"):
        if name in res:
            row[name] = res[name]
    assert row["variants_equal"], "the two variants of the place pass disagree"
    assert res.get("host_model_equal", True), "the host model disagrees with the library"
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=1.0, help="FASTA size of the other pools' inputs")
    ap.add_argument("--gb-distinct", type=float, default=0.05, help="FASTA size of the all-distinct input")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pools", default="0")
    ap.add_argument("--host-model", action="store_true", help="also compute the place words with numpy on the host (slow)")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.child:
        child(args.child, args.gb, args.reps, args.host_model)
        return
    rows = []
    for pool in [int(x) for x in args.pools.split(",")]:
        for canonical in (True, False):
            row = measure(args, pool, canonical, args.gb if pool else args.gb_distinct, 1, 0)
            print(json.dumps(row), flush=True)
            rows.append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
