"""The normalise rule of include/kmc.h (kmc_normalize) as tests/normalize_model.py states it, checked against itself -- nested
targets, the extreme permilles, the identity call and its complement, mates, the summary's balance, the rank shift the
selection kernel relies on, a draw that is not degenerate -- and that the inputs of tests/test_normalize_gpu.py hold every
case they are meant to hold, with a count.  Then what needs no GPU of the library and the CLI: the two symbols, a NULL ctx,
the argument errors of --normalize.  CPU only."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import normalize_inputs as ni
import normalize_model as nm
from conftest import ROOT, SAMPLE

EXE = os.path.join(ROOT, "bin", "k-mer-count")


def _mid_depth(counts):
    d = sorted(nm.depth(c, 500)[1] for c in counts)
    return d[len(d) // 2]


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [5, 31, 33])
def test_identities(k, canonical):
    table, reads, names = ni.table_and_reads(k, 3 + k, canonical)
    counts = nm.all_counts(table, canonical, reads, k)
    run = lambda **kw: nm.normalize_reads(table, canonical, reads, k, counts, **kw)
    # the identity call and its complement
    m = run()
    assert m.out == reads and m.origin == list(range(len(reads))) and all(v == nm.KEEP | nm.EMITTED for v in m.verdict)
    assert m.summary[2:7] == [len(reads), sum(map(len, reads)), 0, 0, 0]
    inv = run(flags=nm.INVERT)
    assert inv.out == [] and inv.offsets == [0] and inv.summary[2:4] == [0, 0] and all(v == nm.KEEP for v in inv.verdict)
    # permille 0 / 1000 against a plain min / max
    lo, hi = run(permille=0), run(permille=1000)
    for c, a, b in zip(counts, lo.stats, hi.stats):
        valid = [x for x in c if x is not None]
        assert a[0] == b[0] == len(valid) and a[1] == (min(valid) if valid else 0) and b[1] == (max(valid) if valid else 0)
    # nested targets for one seed, the summary's balance, INVERT the complement
    T = _mid_depth(counts)
    assert T > 0
    for seed in (0, 7):
        kept = None
        for target in (1, max(T // 3, 2), T, 3 * T, 1 << 40):
            m = run(target=target, min_depth=1, seed=seed)
            s = m.summary
            assert s[2] == s[0] - s[4] - s[5] + s[6] and s[3] == sum(len(reads[r]) for r in m.origin)
            now = {r for r, v in enumerate(m.verdict) if v & nm.KEEP}
            assert kept is None or kept <= now
            kept = now
            inv = run(target=target, min_depth=1, seed=seed, flags=nm.INVERT)
            assert sorted(inv.origin + m.origin) == list(range(len(reads))) and [v & 13 for v in inv.verdict] == [v & 13 for v in m.verdict]
            assert all(row[3] < target < row[2] for row, v in zip(m.stats, m.verdict) if v & nm.DEEP and v & nm.KEEP)
        assert m.summary[5] == 0                                  # (a target above every depth samples nothing down)
    with pytest.raises(AssertionError):
        run(permille=1001)
    with pytest.raises(AssertionError):
        run(flags=4)
    with pytest.raises(AssertionError):
        nm.normalize_reads(table, canonical, reads[:3], k, counts[:3], flags=nm.PAIRED)


def test_mates_share_a_verdict():
    k = 31
    table, reads = ni.pairs(k, 5)
    counts = nm.all_counts(table, True, reads, k)
    own = nm.normalize_reads(table, True, reads, k, counts, target=40, min_depth=2, seed=1)
    d = [s[1] for s in own.stats]
    assert d[:12] == [100, 4, 4, 100, 4, 4, 100, 0, 0, 4, 0, 0] and all(x == 100 for x in d[12:])
    for flags in (nm.PAIRED, nm.PAIRED | nm.INVERT):
        m = nm.normalize_reads(table, True, reads, k, counts, target=40, min_depth=2, seed=1, flags=flags)
        assert all(m.verdict[i] == m.verdict[i + 1] and m.stats[i][2:] == m.stats[i + 1][2:] for i in range(0, len(reads), 2))
        assert [s[2] for s in m.stats[:12]] == [4, 4, 4, 4, 4, 4, 0, 0, 0, 0, 0, 0]
        bits = [v & 13 for v in m.verdict[:12:2]]
        assert bits == [nm.KEEP, nm.KEEP, nm.KEEP, nm.LOW, nm.LOW, nm.LOW]
        deep = [v for v in m.verdict[12::2]]
        assert all(v & nm.DEEP for v in deep) and 0 < sum(1 for v in deep if v & nm.KEEP) < len(deep)
        assert all(bool(v & nm.EMITTED) == (bool(v & nm.KEEP) != bool(flags & nm.INVERT)) for v in m.verdict)
    # a deep read beside a shallow mate is sampled on its own, kept whole in a pair
    assert own.verdict[0] & nm.DEEP and not own.verdict[1] & nm.DEEP


def test_the_rank_shift():
    """the q-th smallest valid count is the (q + I)-th smallest of all W entries once the I invalid ones are written as 0"""
    rng = np.random.default_rng(11)
    for permille in (0, 1, 499, 500, 501, 999, 1000):
        for _ in range(300):
            W = int(rng.integers(1, 80))
            c = [None if rng.random() < 0.3 else int(rng.integers(0, 3)) * int(rng.integers(0, 1 << 32)) for _ in range(W)]
            V, d = nm.depth(c, permille)
            if V:
                flat = sorted(0 if x is None else x for x in c)
                assert flat[((V - 1) * permille) // 1000 + (W - V)] == d


def test_the_draw_is_not_degenerate():
    n = 4096
    worst = 0.0
    for seed in (0, 1, 12345):
        for D, target in ((100, 25), (8, 2), (1000, 10), (3, 1)):
            us = [nm.draw(seed, g, D) for g in range(n)]
            assert all(0 <= u < D for u in us)
            kept = sum(1 for u in us if u < target)
            p = target / D
            dev = abs(kept - n * p) / math.sqrt(n * p * (1 - p))
            worst = max(worst, dev)
            assert dev <= 4.5, (seed, D, target, kept, dev)
    assert worst > 0.5          # (twelve exact hits would be as suspicious)
    assert all(nm.draw(s, g, 0) == 0 for s in (0, 9) for g in range(50))
    assert len({nm.draw(0, g, 1 << 32) for g in range(1000)}) == 1000 and nm.draw(0, 0, 1 << 32) != nm.draw(1, 0, 1 << 32)


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [5, 31, 33])
def test_the_gpu_inputs_hold_their_cases(k, canonical):
    seen_bytes = {}
    for variant in ni.VARIANTS if k == 31 else ("spread",):
        table, reads, names = ni.table_and_reads(k, 3 + k, canonical, variant)
        counts = nm.all_counts(table, canonical, reads, k)
        W = lambda name: len(counts[names[name]])
        V = lambda name: sum(x is not None for x in counts[names[name]])
        # the lengths: below k, every window count of the list, both sides of the variant boundary, a workgroup read off 256
        assert [W("w%d" % n) for n in ni.WINDOWS] == list(ni.WINDOWS) and all(V("w%d" % n) == n for n in ni.WINDOWS)
        assert {ni.WAVE_MAX - 1, ni.WAVE_MAX, ni.WAVE_MAX + 1} <= set(ni.WINDOWS) and {1, 2, 63, 64, 65} <= set(ni.WINDOWS)
        assert max(ni.WINDOWS) > ni.WAVE_MAX + 1 and max(ni.WINDOWS) % 256 and len(reads[names["short"]]) == k - 1
        # the contents
        assert W("all_N") > 0 and V("all_N") == 0
        assert 0 < V("holes") < W("holes") <= ni.WAVE_MAX and W("holes") - V("holes") >= k + 4
        assert ni.WAVE_MAX < W("holes_long") and W("holes_long") - V("holes_long") >= k + 3
        assert V("absent") == W("absent") > 0 and not any(counts[names["absent"]])
        assert [reads[names[n]] for n in ("empty", "empty2", "empty3")] == ["", "", ""] and names["empty3"] == len(reads) - 1
        # the counts: two keys above 32 bits, a depth that saturates
        assert sum(1 for c in table.values() if c == ni.BIG) == 2
        assert nm.depth(counts[names["big"]], 1000)[1] == nm.SAT
        vals = sorted(set(c for c in table.values() if c != ni.BIG))
        seen_bytes[variant] = [len({(c >> s) & 255 for c in vals}) for s in (24, 16, 8, 0)]
        # every permille picks another window of the longest read
        ranks = {((ni.WINDOWS[-1] - 1) * p) // 1000 for p in ni.PERMILLES}
        assert len(ranks) == len(ni.PERMILLES)
    assert all(n > 100 for n in seen_bytes["spread"])
    if k == 31:
        assert seen_bytes["top"] == [256, 1, 1, 1] and seen_bytes["low"] == [1, 1, 1, 256] and seen_bytes["ties"] == [3, 1, 1, 1]
        # ties: one value in most windows, so the median of a long read sits inside a run of equal counts
        table, reads, names = ni.table_and_reads(k, 3 + k, canonical, "ties")
        c = nm.window_counts(reads[names["w2471"]], k, canonical, table)
        assert sum(1 for x in c if x == 7) > len(c) // 2
    # pairs: every combination of mates, deep units kept and dropped
    table, reads = ni.pairs(31, 5)
    assert len(reads) == 52 and len(table) > 1500


def test_the_library_has_the_calls(kmc):
    L = kmc.lib()
    assert "kmc_normalize" in kmc.ABI_SYMBOLS and "kmc_normalize_device" in kmc.ABI_SYMBOLS
    assert L.kmc_normalize and L.kmc_normalize_device
    assert (kmc.NORMALIZE_WORDS, kmc.NORMALIZE_READ_WORDS, kmc.NORM_PAIRED, kmc.NORM_INVERT) == (8, 4, nm.PAIRED, nm.INVERT)
    assert (kmc.NORM_KEEP, kmc.NORM_EMITTED, kmc.NORM_LOW, kmc.NORM_DEEP) == (nm.KEEP, nm.EMITTED, nm.LOW, nm.DEEP)
    no, nb = C.c_uint64(7), C.c_uint64(7)
    assert L.kmc_normalize(None, 500, 0, 0, 0, 0, None, None, 0, None, 0, None, None, 0, None, None, C.byref(no), C.byref(nb), None) == kmc.ERR_ARG
    assert (no.value, nb.value) == (0, 0)
    no, nb = C.c_uint64(7), C.c_uint64(7)
    assert L.kmc_normalize_device(None, 500, 0, 0, 0, 0, None, None, 0, 0, None, None, None, None, None, C.byref(no), C.byref(nb), None) == kmc.ERR_ARG
    assert (no.value, nb.value) == (0, 0)
    s = kmc.NormalizeSummary.from_words(range(8))
    assert s.words() == list(range(8)) and s.emitted == 2 and s.deep_kept == 6 and s.to_text().startswith("reads\t0\nvalid_windows\t1\n")
    r = kmc.NormalizedReads(np.frombuffer(b"ACGTA", np.uint8), np.array([0, 2, 2, 5], np.uint64), np.array([1, 2, 4], np.uint64),
                            np.arange(20, dtype=np.uint32).reshape(5, 4), np.zeros(5, np.uint8), s)
    assert len(r) == 3 and r.strings() == ["AC", "", "GTA"] and r.to_fasta() == ">1 4 5 6\nAC\n>2 8 9 10\n\n>4 16 17 18\nGTA\n"


def test_cli_argument_errors():
    run = lambda *a: subprocess.run([EXE, SAMPLE] + list(a), capture_output=True, text=True)
    norm = ("-k", "31", "--normalize", SAMPLE, "--target", "5")
    assert run("--normalize", SAMPLE, "--target", "5").returncode == 2                              # needs -k
    r = run("-k", "31", "--normalize", SAMPLE)
    assert r.returncode == 2 and "--target" in r.stderr and r.stdout == ""                        # needs --target
    assert run(*norm, "--depth-permille", "1001").returncode == 2
    assert run(*norm, "--depth-permille", "x").returncode == 2 and run(*norm, "--seed", "-1").returncode == 2
    assert run(*norm[:4], "--target").returncode == 2 and run(*norm, "--min-depth").returncode == 2     # a value is missing
    for alone in (["--target", "5"], ["--depth-permille", "500"], ["--min-depth", "2"], ["--seed", "1"], ["--norm-paired"], ["--norm-invert"]):
        r = run("-k", "31", *alone)
        assert r.returncode == 2 and "--normalize FILE" in r.stderr, alone                         # a normalise option without --normalize
    # --invert and --paired keep meaning trim's, with their present errors
    r = run(*norm, "--invert")
    assert r.returncode == 2 and "--trim FILE" in r.stderr
    r = run(*norm, "--paired", "both")
    assert r.returncode == 2 and "--trim FILE" in r.stderr
    for other in (["--correct", SAMPLE], ["--map", SAMPLE], ["--profile", SAMPLE], ["--query-kmers", SAMPLE], ["--trim", SAMPLE],
                  ["--with", SAMPLE, "--compare"], ["--histo", "5"], ["--graph"], ["--components"], ["--variants"]):
        r = run(*norm, *other)
        assert r.returncode == 2 and r.stdout == "", other
