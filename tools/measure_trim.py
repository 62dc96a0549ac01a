#!/usr/bin/env python3
"""Time kmc_trim_device: the mark pass, the run reduction, the verdict / layout passes and the gather, beside
what they are compared with.

Tables, k = 31, canonical and forward: synth pool 0 (every line fresh random: all-distinct, --gb-distinct GB of FASTA).  The
batch that is trimmed is the batch that was counted with one substitution injected per --every bases (default 100).  Range
(1, 0): a window is strong iff its key is in the table.  Per table, in a child process with KMC_UNITIG_TRACE set so that the
library prints its own event times:
  * kmc_profile_device and kmc_correct_device on the same batch and view: the same walk and the same lookups as the mark
    pass (3 warm-up and --reps timed calls; the correct call's own mark_ms from its trace line);
  * kmc_trim_device with KMC_TRIM_LONGEST and with KMC_TRIM_NONE (everything emitted: the gather's worst case): mark_ms,
    reduce_ms, layout_ms, gather_ms of the trace line and the whole call from event pairs;
  * the gather's traffic -- bytes read plus bytes written, from the emitted bases -- over gather_ms, beside the read rate
    kmc_read_peak_device measures in the same process;
  * the existing calls, for the comparison with the parent commit: kmc_profile_device, kmc_correct_device and the place pass
    of kmc_unitig_map_device on the batch as it was counted (none runs new code);
  * with --host-model: the same LONGEST result from kmc_profile's window counts copied out, numpy run-finding and a repack
    on the host, timed with the wall clock and compared with the library's.
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
WARM = 3
HBM_PEAK = 8e12   # bytes / s


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


def host_longest(win, bases, offs, k):
    """(out bases, out offsets, origin) of KMC_TRIM_LONGEST at range (1, 0) from kmc_profile's window counts (per window START;
    a window that is not valid, the last k - 1 positions of a read among them, has the count 0 there, like one whose key is
    absent): numpy run-finding over the batch, a Python repack"""
    o = offs.astype(np.int64)
    n = len(bases)
    strong = win > 0
    is_start = np.zeros(n + 1, bool)
    is_start[o[:-1][o[:-1] < n]] = True
    prev = np.r_[False, strong[:-1]] & ~is_start[:n]
    nxt = np.r_[strong[1:], False] & ~is_start[1:]
    a, b = np.flatnonzero(strong & ~prev), np.flatnonzero(strong & ~nxt)
    ln = b - a + 1
    rid = np.searchsorted(o, a, side="right") - 1
    # the longest run per read, the first among equals: sort by (read, -length, start)
    order = np.lexsort((a, -ln, rid))
    first = np.r_[True, rid[order][1:] != rid[order][:-1]]
    pick = order[first]
    pick = pick[np.argsort(rid[pick])]
    parts, oo = [], [0]
    for s, m in zip(a[pick].tolist(), ln[pick].tolist()):
        parts.append(bases[s:s + m + k - 1])
        oo.append(oo[-1] + m + k - 1)
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), np.array(oo, np.uint64), rid[pick].astype(np.uint64)


def child(spec, gb, reps, every, host_model):
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
        g = torch.Generator(device="cpu").manual_seed(7)
        at = torch.arange(0, n_bases - every + 1, every) + torch.randint(0, max(every - k - 1, 1), ((n_bases - every) // every + 1,), generator=g)
        at = at.to(dev)
        nxt = torch.arange(256, dtype=torch.uint8)
        for x, y in zip(b"ACGT", b"CGTA"):
            nxt[x] = y
        d_e = d_b.clone()
        d_e[at] = nxt.to(dev)[d_b[at].long()]
        stream.synchronize()
        clean = (d_b.data_ptr(), d_o.data_ptr(), n_rec, n_bases)
        batch = (d_e.data_ptr(), d_o.data_ptr(), n_rec, n_bases)
        d_win = torch.zeros(n_bases, dtype=torch.int32, device=dev)
        d_st = torch.zeros((n_rec, kmc.PROFILE_WORDS), dtype=torch.int64, device=dev)
        os.environ.pop("KMC_UNITIG_TRACE", None)

        def timed(f):
            for _ in range(WARM):
                f()
            return [ev_ms(stream, f) for _ in range(reps)]
        out["profile_ms"] = timed(lambda: kc.profile_device(batch[0], batch[1], n_rec, n_bases, 1, d_win.data_ptr(), d_st.data_ptr()))
        out["profile_clean_ms"] = timed(lambda: kc.profile_device(clean[0], clean[1], n_rec, n_bases, 1, d_win.data_ptr(), d_st.data_ptr()))
        out["correct_clean_ms"] = timed(lambda: kc.correct_reads_device(*clean, lo_c, hi_c))
        for _ in range(WARM):
            kc.correct_reads_device(*batch, lo_c, hi_c)
        os.environ["KMC_UNITIG_TRACE"] = "1"
        print("mark correct", file=sys.stderr, flush=True)
        out["correct_ms"] = [ev_ms(stream, lambda: kc.correct_reads_device(*batch, lo_c, hi_c)) for _ in range(reps)]
        res = {}
        for name, mode in (("longest", kmc.TRIM_LONGEST), ("none", kmc.TRIM_NONE)):
            os.environ.pop("KMC_UNITIG_TRACE", None)
            for _ in range(WARM):
                kc.trim_reads_device(*batch, lo_c, hi_c, mode)
            os.environ["KMC_UNITIG_TRACE"] = "1"
            print("mark trim_" + name, file=sys.stderr, flush=True)
            out["call_%s_ms" % name] = [ev_ms(stream, lambda: res.update({name: kc.trim_reads_device(*batch, lo_c, hi_c, mode)})) for _ in range(reps)]
            out["summary_" + name] = res[name][7].words()
        os.environ.pop("KMC_UNITIG_TRACE", None)
        # the read rate of this process, on a buffer the size of the batch
        peak_ms, _ = kmc.read_peak_device(d_e.data_ptr(), n_bases // 16 * 16, 0, stream.cuda_stream)
        out["read_peak_bytes_per_s"] = (n_bases // 16 * 16) / (peak_ms * 1e-3)
        db, doo, dorg, ds, dv, no, nb, _ = res["none"]
        out["none_is_identity"] = bool(np.array_equal(dev_words(db, nb, dev), d_e[:n_bases].cpu().numpy())) and no == n_rec
        kc.unitigs_device(lo_c, hi_c)
        for _ in range(WARM):
            kc.map_reads_device(*clean, lo_c, hi_c)
        os.environ["KMC_UNITIG_TRACE"] = "1"
        print("mark map", file=sys.stderr, flush=True)
        for _ in range(reps):
            kc.map_reads_device(*clean, lo_c, hi_c)
        print("mark end", file=sys.stderr, flush=True)
        os.environ.pop("KMC_UNITIG_TRACE", None)
        out["keys"], out["reads"], out["bases"], out["errors"] = nd, n_rec, n_bases, int(at.numel())
        if host_model:
            db, doo, dorg, ds, dv, no, nb, _ = kc.trim_reads_device(*batch, lo_c, hi_c, kmc.TRIM_LONGEST)
            got = (dev_words(db, nb, dev), dev_words(doo, 8 * (no + 1), dev).view(np.uint64), dev_words(dorg, 8 * no, dev).view(np.uint64))
            ho = d_o.cpu().numpy().astype(np.uint64)
            t0 = time.perf_counter()
            kc.profile_device(batch[0], batch[1], n_rec, n_bases, 1, d_win.data_ptr(), 0)
            kc.sync()
            win = d_win.cpu().numpy().view(np.uint32)
            hb = d_e[:n_bases].cpu().numpy()
            want = host_longest(win, hb, ho, k)
            out["host_model_s"] = time.perf_counter() - t0
            out["host_model_equal"] = all(np.array_equal(a, b) for a, b in zip(want, got))
        kc.close()
    print(json.dumps(out), flush=True)


def parse(line):
    return {name: float(val) if "." in val else int(val) for name, val in re.findall(r"(\w+) ([\d.]+)", line.split(":", 1)[1])}


def med_min(xs):
    return dict(median=float(np.median(xs)), min=float(min(xs)))


def measure(args, pool, canonical, gb, lo_c, hi_c, k=31):
    env = dict(os.environ)
    env.pop("KMC_UNITIG_TRACE", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", f"{pool},{int(canonical)},{k},{lo_c},{hi_c}", "--gb", str(gb), "--reps", str(args.reps),
           "--every", str(args.every)]
    r = subprocess.run(cmd + (["--host-model"] if args.host_model else []), capture_output=True, text=True, env=env)
    if r.returncode:                            # nothing more is started on a device where a process has just failed
        raise RuntimeError("the traced child failed (exit %d): %s" % (r.returncode, r.stderr[-600:]))
    res = json.loads(r.stdout.strip().splitlines()[-1])
    sect, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("mark "):
            cur = line[5:]
            sect[cur] = []
        elif cur and line.startswith("kmc_"):
            sect[cur].append(line)
    row = dict(table=f"pool{pool}_k{k}_{'canonical' if canonical else 'forward'} ({gb:g} GB, {res['keys']} keys)", range=[lo_c, hi_c],
               keys=res["keys"], reads=res["reads"], bases=res["bases"], errors=res["errors"], none_is_identity=res["none_is_identity"],
               profile_ms=med_min(res["profile_ms"]), profile_clean_ms=med_min(res["profile_clean_ms"]), correct_ms=med_min(res["correct_ms"]),
               correct_clean_ms=med_min(res["correct_clean_ms"]), read_peak_bytes_per_s=res["read_peak_bytes_per_s"])
    row["correct_mark_ms"] = med_min([parse(l)["mark_ms"] for l in sect["correct"] if l.startswith("kmc_correct:")])
    row["map_place_ms"] = med_min([parse(l)["place_ms"] for l in sect["map"] if l.startswith("kmc_unitig_map:")])
    for name in ("longest", "none"):
        lines = [parse(l) for l in sect["trim_" + name] if l.startswith("kmc_trim:")]
        assert len(lines) == args.reps, sect["trim_" + name]
        t = dict(summary=res["summary_" + name], call_ms=med_min(res["call_%s_ms" % name]))
        for ph in ("mark_ms", "reduce_ms", "layout_ms", "gather_ms"):
            t[ph] = med_min([l[ph] for l in lines])
        t["behind_mark_ms"] = float(np.median([l["reduce_ms"] + l["layout_ms"] + l["gather_ms"] for l in lines]))
        t["behind_mark_over_mark"] = t["behind_mark_ms"] / t["mark_ms"]["median"]
        # the gather reads every emitted base once (two aligned 16-byte loads per 16 bytes touch each source byte at most
        # twice, the second time from cache) and writes it once; out_offsets and src add 16 bytes per emitted read
        gb_moved = 2 * t["summary"][5] + 16 * t["summary"][4]
        t["gather_bytes_per_s"] = gb_moved / (t["gather_ms"]["median"] * 1e-3)
        t["gather_of_hbm_peak"] = t["gather_bytes_per_s"] / HBM_PEAK
        t["gather_of_read_peak"] = t["gather_bytes_per_s"] / res["read_peak_bytes_per_s"]
        row[name] = t
    row["mark_over_profile"] = row["longest"]["mark_ms"]["median"] / row["profile_ms"]["median"]
    row["mark_over_correct_mark"] = row["longest"]["mark_ms"]["median"] / row["correct_mark_ms"]["median"]
    for name in ("host_model_s", "host_model_equal"):
        if name in res:
            row[name] = res[name]
    assert res["none_is_identity"], "KMC_TRIM_NONE did not return the batch"
    assert res.get("host_model_equal", True), "the host model disagrees with the library"
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb-distinct", type=float, default=0.05, help="FASTA size of the all-distinct input")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--every", type=int, default=100, help="one substitution per this many bases")
    ap.add_argument("--host-model", action="store_true", help="also trim the batch with numpy on the host (slow)")
    ap.add_argument("--gb", type=float, default=0.05, help=argparse.SUPPRESS)
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.child:
        child(args.child, args.gb, args.reps, args.every, args.host_model)
        return
    rows = []
    for canonical in (True, False):
        row = measure(args, 0, canonical, args.gb_distinct, 1, 0)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
