#!/usr/bin/env python3
"""Time kmc_normalize_device: the profile pass, the selection, the verdict / layout passes and the gather,
beside what they are compared with.

Tables, k = 31, canonical and forward: synth pool 0 (every line fresh random: all-distinct, --gb-distinct GB of FASTA).  The
batch is counted once and its first half a second time, so the keys are the all-distinct table's and half the reads have
depth 2, the others depth 1: with permille 500 and target 1 half the reads are DEEP and each of those is kept with
probability 1 / 2.  The batch that is normalised is the batch that was counted.  Per table, in a child process with
KMC_UNITIG_TRACE set so that the library prints its own event times:
  * kmc_profile_device on the same batch and view, both outputs (3 warm-up and --reps timed calls);
  * kmc_normalize_device: profile_ms, select_ms, layout_ms, gather_ms of the trace line and the whole call from event pairs;
  * with --spread: the same once more after a random 32-bit count was merged onto every key (counts that differ in all four
    bytes: the selection then walks 32 bits instead of 2), target 2^31;
  * with --host-model: the same result from kmc_profile's window counts copied out, a numpy per-read selection, the verdict
    in numpy and a repack on the host, timed with the wall clock and compared word for word with the library's.
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
U64 = np.uint64


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


def host_normalize(win, valid, bases, offs, k, permille, target, min_depth, seed):
    """(out bases, out offsets, origin, stats, verdict) of kmc_normalize without flags from kmc_profile's window counts (per
    window START; a window that is not valid has the count 0 there) and its valid-window counts per read: the I invalid
    entries of a read sort to the front, so the q-th smallest valid count is entry q + I of the read's sorted windows"""
    o = offs.astype(np.int64)
    n = len(o) - 1
    lens = o[1:] - o[:-1]
    W = np.maximum(lens - k + 1, 0)
    V = valid.astype(np.int64)
    rank = np.where(V > 0, ((V - 1) * permille) // 1000 + (W - V), 0)
    d = np.zeros(n, U64)
    if n and (lens == lens[0]).all() and W[0] > 0:
        rows = np.sort(win.reshape(n, int(lens[0]))[:, :int(W[0])], axis=1)
        d = np.where(V > 0, np.take_along_axis(rows, rank[:, None], axis=1)[:, 0], 0).astype(U64)
    else:
        for r in np.flatnonzero(V > 0).tolist():
            d[r] = np.partition(win[o[r]:o[r] + W[r]], rank[r])[rank[r]]
    with np.errstate(over="ignore"):
        x = U64(seed) + (np.arange(n, dtype=U64) + U64(1)) * U64(0x9E3779B97F4A7C15)
        x ^= x >> U64(30)
        x *= U64(0xBF58476D1CE4E5B9)
        x ^= x >> U64(27)
        x *= U64(0x94D049BB133111EB)
        x ^= x >> U64(31)
        u = ((x >> U64(32)) * d) >> U64(32)
    low = d < U64(min_depth)
    deep = ~low & (d > U64(target)) if target else np.zeros(n, bool)
    keep = ~low & (~deep | (u < U64(target)))
    verdict = (keep * 3 + low * 4 + deep * 8).astype(np.uint8)
    stats = np.stack([V.astype(U64), d, d, u], axis=1).astype(np.uint32)
    out = bases[np.repeat(keep, lens)]
    oo = np.zeros(int(keep.sum()) + 1, U64)
    oo[1:] = np.cumsum(lens[keep])
    return out, oo, np.flatnonzero(keep).astype(U64), stats, verdict


def run_config(kc, stream, dev, batch, reps, rule, tag, out):
    """the traced calls of one rule; returns the last result"""
    n_rec, n_bases = batch[2], batch[3]
    res = {}
    os.environ.pop("KMC_UNITIG_TRACE", None)
    for _ in range(WARM):
        kc.normalize_reads_device(*batch, **rule)
    os.environ["KMC_UNITIG_TRACE"] = "1"
    print("mark normalize_" + tag, file=sys.stderr, flush=True)
    out["call_%s_ms" % tag] = [ev_ms(stream, lambda: res.update(r=kc.normalize_reads_device(*batch, **rule))) for _ in range(reps)]
    print("mark end", file=sys.stderr, flush=True)
    os.environ.pop("KMC_UNITIG_TRACE", None)
    out["summary_" + tag] = res["r"][7].words()
    return res["r"]


def child(spec, gb, reps, host_model, spread):
    pool, canonical, k = [int(x) for x in spec.split(",")]
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
        half = n_rec // 2
        kc.add_batch_device(d_b.data_ptr(), d_o.data_ptr(), half, half * s.read_len, s.read_len)
        nd, _ = kc.finalize()
        batch = (d_b.data_ptr(), d_o.data_ptr(), n_rec, n_bases)
        d_win = torch.zeros(n_bases, dtype=torch.int32, device=dev)
        d_st = torch.zeros((n_rec, kmc.PROFILE_WORDS), dtype=torch.int64, device=dev)
        os.environ.pop("KMC_UNITIG_TRACE", None)
        prof = lambda: kc.profile_device(batch[0], batch[1], n_rec, n_bases, 1, d_win.data_ptr(), d_st.data_ptr())
        for _ in range(WARM):
            prof()
        out["profile_ms"] = [ev_ms(stream, prof) for _ in range(reps)]
        rule = dict(target=1, permille=500, min_depth=0, seed=1)
        db, doo, dorg, ds, dv, no, nb, _ = run_config(kc, stream, dev, batch, reps, rule, "main", out)
        out["keys"], out["reads"], out["bases"] = nd, n_rec, n_bases
        if host_model:
            got = (dev_words(db, nb, dev), dev_words(doo, 8 * (no + 1), dev).view(U64), dev_words(dorg, 8 * no, dev).view(U64),
                   dev_words(ds, 16 * n_rec, dev).view(np.uint32).reshape(n_rec, 4), dev_words(dv, n_rec, dev))
            ho = d_o.cpu().numpy().astype(U64)
            t0 = time.perf_counter()
            prof()
            kc.sync()
            win = d_win.cpu().numpy().view(np.uint32)
            valid = d_st.cpu().numpy().view(U64)[:, 0]
            hb = d_b[:n_bases].cpu().numpy()
            want = host_normalize(win, valid, hb, ho, k, rule["permille"], rule["target"], rule["min_depth"], rule["seed"])
            out["host_model_s"] = time.perf_counter() - t0
            out["host_model_equal"] = all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(want, got))
        if spread:
            # a random 32-bit count onto every key of the view (the keys copied first: the merge rewrites the table the view
            # came from, and the next finalize the view)
            d_hi, d_lo, d_cnt, n = kc.export_device()
            lo = kd.device_view(d_lo, n, dev).clone()
            g = torch.Generator(device="cpu").manual_seed(11)
            add = torch.randint(1, 1 << 32, (n,), generator=g, dtype=torch.int64).to(dev)
            stream.synchronize()
            kc.merge_pairs_device(0, lo.data_ptr(), add.data_ptr(), n)
            nd2, _ = kc.finalize()
            assert nd2 == nd
            for _ in range(WARM):
                prof()
            out["profile_spread_ms"] = [ev_ms(stream, prof) for _ in range(reps)]
            run_config(kc, stream, dev, batch, reps, dict(target=1 << 31, permille=500, min_depth=0, seed=1), "spread", out)
        kc.close()
    print(json.dumps(out), flush=True)


def parse(line):
    return {name: float(val) if "." in val else int(val) for name, val in re.findall(r"(\w+) ([\d.]+)", line.split(":", 1)[1])}


def med_min(xs):
    return dict(median=float(np.median(xs)), min=float(min(xs)))


def measure(args, pool, canonical, gb, k=31):
    env = dict(os.environ)
    env.pop("KMC_UNITIG_TRACE", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", f"{pool},{int(canonical)},{k}", "--gb", str(gb), "--reps", str(args.reps)]
    cmd += (["--host-model"] if args.host_model else []) + (["--spread"] if args.spread else [])
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
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
    row = dict(table=f"pool{pool}_k{k}_{'canonical' if canonical else 'forward'} ({gb:g} GB, {res['keys']} keys)", keys=res["keys"],
               reads=res["reads"], bases=res["bases"], profile_ms=med_min(res["profile_ms"]))
    for tag in ("main", "spread"):
        if "summary_" + tag not in res:
            continue
        lines = [parse(l) for l in sect["normalize_" + tag] if l.startswith("kmc_normalize:")]
        assert len(lines) == args.reps, sect["normalize_" + tag]
        t = dict(summary=res["summary_" + tag], call_ms=med_min(res["call_%s_ms" % tag]))
        for ph in ("profile_ms", "select_ms", "layout_ms", "gather_ms"):
            t[ph] = med_min([l[ph] for l in lines])
        t["select_over_profile"] = t["select_ms"]["median"] / t["profile_ms"]["median"]
        t["behind_profile_ms"] = float(np.median([l["select_ms"] + l["layout_ms"] + l["gather_ms"] for l in lines]))
        t["deep_share"] = t["summary"][5] / max(t["summary"][0], 1)
        row[tag] = t
    if "profile_spread_ms" in res:
        row["profile_spread_ms"] = med_min(res["profile_spread_ms"])
    row["profile_pass_over_profile_call"] = row["main"]["profile_ms"]["median"] / row["profile_ms"]["median"]
    if "host_model_s" in res:
        row["host_model_s"], row["host_model_equal"] = res["host_model_s"], res["host_model_equal"]
        row["host_over_call"] = res["host_model_s"] * 1e3 / row["main"]["call_ms"]["median"]
    assert res.get("host_model_equal", True), "the host model disagrees with the library"
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb-distinct", type=float, default=0.05, help="FASTA size of the all-distinct input")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-model", action="store_true", help="also normalise the batch with numpy on the host (slow)")
    ap.add_argument("--spread", action="store_true", help="also with random 32-bit counts on every key")
    ap.add_argument("--gb", type=float, default=0.05, help=argparse.SUPPRESS)
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.child:
        child(args.child, args.gb, args.reps, args.host_model, args.spread)
        return
    rows = []
    for canonical in (True, False):
        row = measure(args, 0, canonical, args.gb_distinct)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
