#!/usr/bin/env python3
"""Time kmc_correct_device: the mark pass, the run passes and the try pass, beside what they are compared with.

Tables, k = 31, canonical and forward: synth pool 0 (every line fresh random: all-distinct, --gb-distinct GB of FASTA).  The
batch that is corrected is the batch that was counted with one substitution injected per --every bases (default 100: more
than k apart, so every error is one candidate and the try pass issues about as many lookups as the mark pass).  Range
(1, 0): a window is weak iff its key is not in the table.  Per table, in a child process with KMC_UNITIG_TRACE set so that
the library prints its own event times:
  * kmc_profile_device on the same batch and view, timed with event pairs on the ctx's stream: the same walk and the same
    lookups as the mark pass (3 warm-up and --reps timed calls, median and minimum);
  * kmc_correct_device: mark_ms, runs_ms, try_ms of the trace line and the whole call from event pairs, the same way;
  * the existing calls, for the comparison with the parent commit: kmc_profile_device on the batch as it was counted and the
    place pass of kmc_unitig_map_device (neither runs new code);
  * with --host-model: the same corrected batch and summary from numpy on the host (keys of all windows, a search in the
    sorted table, runs and candidates by array arithmetic), timed with the wall clock and compared with the library's.
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


def host_correct(table_keys, bases, offs, k, canonical):
    """(corrected bases, summary words) by the definitions of include/kmc.h in numpy, range (1, 0), no empty reads"""
    u64 = np.uint64
    lut = np.full(256, 4, np.uint8)
    lut[[65, 67, 71, 84]] = [0, 1, 2, 3]
    codes = lut[bases]
    valid = codes < 4
    n = len(bases)
    o = offs.astype(np.int64)
    starts = np.zeros(n + 1, np.int64)
    np.add.at(starts, o, 1)
    rid = np.cumsum(starts[:n]) - 1
    is_start = starts[:n] > 0
    pos = np.arange(n)
    c64 = np.where(valid, codes, 0).astype(u64)
    fw, rc, ok = _keys(c64, valid, k)
    ok &= pos + k <= o[rid + 1]

    def present(f, r):
        key = np.minimum(f, r) if canonical else f
        at = np.minimum(np.searchsorted(table_keys, key), max(len(table_keys) - 1, 0))
        return table_keys[at] == key if len(table_keys) else np.zeros(len(key), bool)
    solid = present(fw, rc)
    weak, strong = ok & ~solid, ok & solid
    prev_weak = np.r_[False, weak[:-1]] & ~is_start
    next_weak = np.r_[weak[1:], False] & ~np.r_[is_start[1:], True]
    a, b = np.flatnonzero(weak & ~prev_weak), np.flatnonzero(weak & ~next_weak)
    ln = b - a + 1
    first, last = o[rid[a]], o[rid[a] + 1] - k
    l_start, r_end = a == first, b == last
    l_solid = ~l_start & strong[np.maximum(a - 1, 0)]
    r_solid = ~r_end & strong[np.minimum(b + 1, n - 1)]
    interior, head, tail = l_solid & r_solid & (ln == k), l_start & r_solid & (ln <= k), l_solid & r_end & (ln <= k)
    is_c = interior | head | tail
    p = np.where(tail, a + k - 1, b)[is_c]
    a, ln = a[is_c], ln[is_c]
    # every (candidate, window) pair, then the three replacements
    cid = np.repeat(np.arange(len(a)), ln)
    cut = np.r_[0, np.cumsum(ln)[:-1]]
    j = a[cid] + (np.arange(len(cid)) - cut[cid])
    i = (p[cid] - j).astype(u64)
    old = c64[p]
    accepted = np.zeros((len(a), 4), bool)
    for t in (1, 2, 3):
        new = (old + u64(t)) & u64(3)
        d = (old ^ new)[cid]
        f2 = fw[j] ^ (d << (u64(2) * (u64(k - 1) - i)))
        r2 = rc[j] ^ (d << (u64(2) * i))          # (3 - old) ^ (3 - new) == old ^ new
        hit = present(f2, r2)
        accepted[np.arange(len(a)), new.astype(np.int64)] = np.logical_and.reduceat(hit, cut) if len(a) else []
    n_acc = accepted.sum(axis=1)
    fix = n_acc == 1
    out = bases.copy()
    out[p[fix]] = np.frombuffer(b"ACGT", np.uint8)[accepted[fix].argmax(axis=1)]
    n_weak = int(weak.sum())
    words = [len(offs) - 1, int(ok.sum()), n_weak, len(is_c), int(is_c.sum()), int(fix.sum()), int((n_acc > 1).sum()), n_weak - int(ln[fix].sum())]
    return out, words


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
        # the batch with one substitution per `every` bases, at a random place of each stretch (two of them more than k apart): the next base of ACGT
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
        for _ in range(WARM):
            kc.correct_reads_device(*batch, lo_c, hi_c)
        os.environ["KMC_UNITIG_TRACE"] = "1"
        print("mark correct", file=sys.stderr, flush=True)
        res = {}
        out["call_ms"] = [ev_ms(stream, lambda: res.update(r=kc.correct_reads_device(*batch, lo_c, hi_c))) for _ in range(reps)]
        dc, ds, dco, dr, nc, summ = res["r"]
        out["summary"] = summ.words()
        got = dev_words(dc, n_bases, dev)
        out["restored"] = bool(np.array_equal(got, d_b[:n_bases].cpu().numpy()))
        os.environ.pop("KMC_UNITIG_TRACE", None)
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
        if host_model and k <= 31:
            t = kc.export()
            hb, ho = d_e[:n_bases].cpu().numpy(), d_o.cpu().numpy().astype(np.uint64)
            t0 = time.perf_counter()
            want, words = host_correct(np.asarray(t.key_lo), hb, ho, k, bool(canonical))
            out["host_model_s"] = time.perf_counter() - t0
            out["host_model_equal"] = bool(np.array_equal(want, got)) and words == out["summary"]
            out["host_model_summary"] = words
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
    lines = [parse(l) for l in sect["correct"] if l.startswith("kmc_correct:")]
    assert len(lines) == args.reps, sect["correct"]
    places = [parse(l)["place_ms"] for l in sect["map"] if l.startswith("kmc_unitig_map:")]
    row = dict(table=f"pool{pool}_k{k}_{'canonical' if canonical else 'forward'} ({gb:g} GB, {res['keys']} keys)", range=[lo_c, hi_c],
               keys=res["keys"], reads=res["reads"], bases=res["bases"], errors=res["errors"], summary=res["summary"], restored=res["restored"],
               profile_ms=med_min(res["profile_ms"]), profile_clean_ms=med_min(res["profile_clean_ms"]), map_place_ms=med_min(places),
               mark_ms=med_min([l["mark_ms"] for l in lines]), runs_ms=med_min([l["runs_ms"] for l in lines]),
               try_ms=med_min([l["try_ms"] for l in lines]), call_ms=med_min(res["call_ms"]))
    row["mark_over_profile"] = row["mark_ms"]["median"] / row["profile_ms"]["median"]
    row["windows_per_s"] = res["summary"][1] / (row["call_ms"]["median"] * 1e-3)
    for name in ("host_model_s", "host_model_equal", "host_model_summary"):
        if name in res:
            row[name] = res[name]
    assert res.get("host_model_equal", True), "the host model disagrees with the library"
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb-distinct", type=float, default=0.05, help="FASTA size of the all-distinct input")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--every", type=int, default=100, help="one substitution per this many bases")
    ap.add_argument("--host-model", action="store_true", help="also correct the batch with numpy on the host (slow)")
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
