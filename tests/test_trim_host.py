"""The trim rule of include/kmc.h (kmc_trim) as tests/trim_model.py states it, checked against itself -- the identities, the
idempotence of LONGEST and ENDS, the pair and invert truth tables, V and S against correct_model -- and that the inputs of
tests/test_trim_gpu.py hold every case they are meant to hold, with a count.  Then what needs no GPU of the library and the
CLI: the two symbols, a NULL ctx, the argument errors of --trim.  CPU only."""
import ctypes as C
import os
import subprocess

import pytest

import correct_model as cm
import graph_model as gm
import trim_inputs as ti
import trim_model as tm
from conftest import ROOT, SAMPLE

EXE = os.path.join(ROOT, "bin", "k-mer-count")
RANGES = ((1, 0), (2, 0), (2, 3))


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [5, 31, 32])
def test_identities_and_idempotence(k, canonical):
    sample, reads = ti.genome_reads(k, 7 + k)
    table = gm.count_table(sample, k, canonical)
    for lo, hi in RANGES:
        m = tm.trim_reads(table, canonical, reads, lo, hi, mode=tm.NONE)
        assert m.out == reads and m.origin == list(range(len(reads))) and m.summary[4] == len(reads) and m.summary[6] == 0
        assert m.summary[5] == m.summary[7] == sum(map(len, reads)) and all(v == tm.PASS | tm.EMITTED for v in m.verdict)
        inv = tm.trim_reads(table, canonical, reads, lo, hi, mode=tm.NONE, flags=tm.INVERT)
        assert inv.out == [] and inv.offsets == [0] and inv.summary[3] == len(reads) and inv.summary[4:] == [0, 0, 0, 0]
        # V, S against the correction model's per-read words
        c = cm.correct_reads(table, canonical, reads, lo, hi)
        assert [s[:2] for s in m.stats] == [[s[0], s[0] - s[1]] for s in c.stats]
        for mode in (tm.LONGEST, tm.ENDS):
            a = tm.trim_reads(table, canonical, reads, lo, hi, mode=mode)
            b = tm.trim_reads(table, canonical, a.out, lo, hi, mode=mode)
            assert b.out == a.out and b.origin == list(range(len(a.out))) and b.summary[6] == 0
            assert a.summary[4] == a.summary[3] == sum(1 for s in a.stats if s[1]) and a.summary[7] - a.summary[5] >= 0
            if mode == tm.LONGEST:
                assert b.summary[1] == b.summary[2] == sum(len(s) - k + 1 for s in a.out)
            for i, s in zip(a.origin, a.out):
                assert s and s in reads[i] and len(s) >= k
        if k >= 31:
            a = tm.trim_reads(table, canonical, reads, 2, 0, mode=tm.LONGEST)
            assert a.summary[6] >= 30 and 0 < a.summary[4] < len(reads)


def test_pair_and_invert_truth_tables():
    k = 31
    sample, reads = ti.pairs(k, 3)
    table = gm.count_table(sample, k, True)
    own = [True, True, True, False, False, True, False, False] * 2
    rule = dict(mode=tm.NONE, min_strong=1)
    m = tm.trim_reads(table, True, reads, 2, 0, **rule)
    assert [bool(v & tm.PASS) for v in m.verdict] == own and [bool(v & tm.EMITTED) for v in m.verdict] == own
    both = tm.trim_reads(table, True, reads, 2, 0, flags=tm.PAIR_BOTH, **rule)
    assert [bool(v & tm.EMITTED) for v in both.verdict] == [True, True] + [False] * 6 + [True, True] + [False] * 6
    either = tm.trim_reads(table, True, reads, 2, 0, flags=tm.PAIR_EITHER, **rule)
    assert [bool(v & tm.EMITTED) for v in either.verdict] == ([True] * 6 + [False] * 2) * 2
    for flags, base in ((tm.INVERT, m), (tm.INVERT | tm.PAIR_BOTH, both), (tm.INVERT | tm.PAIR_EITHER, either)):
        inv = tm.trim_reads(table, True, reads, 2, 0, flags=flags, **rule)
        assert [v & tm.PASS for v in inv.verdict] == [v & tm.PASS for v in base.verdict]
        assert [bool(v & tm.EMITTED) for v in inv.verdict] == [not v & tm.EMITTED for v in base.verdict]
        assert sorted(inv.origin + base.origin) == list(range(len(reads)))
    for bad in (dict(flags=tm.PAIR_BOTH | tm.PAIR_EITHER), dict(flags=tm.INVERT, mode=tm.ENDS), dict(flags=8), dict(mode=3), dict(min_permille=1001)):
        with pytest.raises(AssertionError):
            tm.trim_reads(table, True, reads, 2, 0, **bad)
    with pytest.raises(AssertionError):
        tm.trim_reads(table, True, reads[:3], 2, 0, flags=tm.PAIR_BOTH)


def test_the_run_shapes_by_name():
    k = 31
    for canonical in (True, False):
        sample, reads, names, d = ti.shapes(k, 5)
        table = gm.count_table(sample, k, canonical)
        w = lambda name: tm.read_words(reads[names[name]], k, canonical, gm.solid_set(table, 2, 0))
        assert w("all_strong")[:6] == (d - 1, d - 1, 0, d - 2, 0, d - 1)
        assert w("none_strong")[:2] == (d - 1, 0)
        assert w("weak_at_0")[:6] == (d, d - 1, 1, d - 1, 1, d - 1)
        assert w("weak_at_last")[:6] == (d, d - 1, 0, d - 2, 0, d - 1)
        assert w("weak_in_the_middle")[:6] == (2 * d - 1, 2 * d - 2, 0, 2 * d - 2, 0, d - 1) and w("weak_in_the_middle")[6] == [(0, d - 1), (d, d - 1)]
        assert w("longest_run_last")[:6] == (d + 5, d + 4, 0, d + 4, 6, d - 1)
        V, S, F, E, B, N, runs = w("split_by_N")
        assert V == S == d - 1 - k and len(runs) == 2 and F == 0 and E == d - 2     # no weak window: the N alone splits the run
        V, S, F, E, B, N, runs = w("ends_with_weak_inside")
        assert (V - S, F, E, len(runs)) == (3, 0, len(reads[names["ends_with_weak_inside"]]) - k, 4)
        m = tm.trim_reads(table, canonical, reads, 2, 0, mode=tm.ENDS)
        assert m.out[m.origin.index(names["ends_with_weak_inside"])] == reads[names["ends_with_weak_inside"]]
        assert names["none_strong"] not in m.origin


def test_the_gpu_inputs_hold_their_cases():
    k = 31
    # seams: runs that begin and end at bits 63, 0 and 1 of a word and on both sides of the chunk edges
    sample, reads = ti.seams(k, 7)
    table = gm.count_table(sample, k, True)
    V, S, F, E, B, N, runs = tm.read_words(reads[0], k, True, gm.solid_set(table, 1, 0))
    assert V - S == len(ti.SEAM_WEAK_ENDS) and sum(map(len, reads[:2])) == 3072
    begins, ends = {a + k - 1 for a, n in runs}, {a + n + k - 2 for a, n in runs}      # as window END positions in the batch
    assert {63, 65, 128, 193, 258, 1023, 1025, 2047, 2049} <= begins and {63, 126, 191, 256, 1021, 1023, 2045, 2047} <= ends
    assert sum(1 for a, n in runs if n == 1) == 3
    # the reduce variants: both boundaries from both sides, the longest run across a lane seam and across a wave seam
    sample, reads = ti.variants(k, 9)
    assert [len(r) - k + 1 for r in reads[:6]] == [ti.LANE_MAX - 1, ti.LANE_MAX, ti.LANE_MAX + 1, ti.WAVE_MAX - 1, ti.WAVE_MAX, ti.WAVE_MAX + 1] and [len(r) for r in reads[6:]] == [5000, 70000]
    solid = gm.solid_set(gm.count_table(sample, k, True), 1, 0)
    V, S, F, E, B, N, runs = tm.read_words(reads[6], k, True, solid)
    assert (B, N) == (701, 1900 - k - 700) and len(runs) == 8 and B // 128 != (B + N) // 128
    V, S, F, E, B, N, runs = tm.read_words(reads[7], k, True, solid)
    assert (B, N) == (18001, 22500 - k - 18000) and B < 20480 - 64 - k and B + N > 20480 + 64 and len(runs) > 40
    # alignment: every (length, source, destination) triple
    sample, reads, met = ti.alignment(k, 11)
    assert met == {(n, s, d) for n in ti.GATHER_LENS for s in range(16) for d in range(16)}
    m = tm.trim_reads(gm.count_table(sample, k, True), True, reads, 2, 0, mode=tm.NONE, flags=tm.INVERT, min_strong=1)
    seen, P = set(), 0
    pos = {}
    for i, r in enumerate(reads):
        pos[i] = P
        P += len(r)
    for i, o in zip(m.origin, m.offsets):
        seen.add((len(reads[i]), pos[i] % 16, o % 16))
    assert met <= seen and m.summary[4] == len(reads) - 8 * 256 and sum(1 for s in m.out if not s) >= 5
    blocks = {}
    for o, s in zip(m.offsets, m.out):
        blocks[o // 16] = blocks.get(o // 16, 0) + 1
    assert max(blocks.values()) >= 16
    # many short reads: spans on both sides of every 2048-read scan tile's edge
    sample, reads = ti.many_short(k, 10)
    m = tm.trim_reads(gm.count_table(sample, k, True), True, reads, 2, 0, mode=tm.LONGEST)
    assert len(reads) == 3000 and m.summary[4] >= 2900 and m.summary[6] >= 2900 and len({s[2] for s in m.stats}) >= k


def test_the_library_has_the_calls(kmc):
    L = kmc.lib()
    assert "kmc_trim" in kmc.ABI_SYMBOLS and "kmc_trim_device" in kmc.ABI_SYMBOLS
    assert L.kmc_trim and L.kmc_trim_device
    assert (kmc.TRIM_WORDS, kmc.TRIM_READ_WORDS, kmc.TRIM_NONE, kmc.TRIM_ENDS, kmc.TRIM_LONGEST) == (8, 4, tm.NONE, tm.ENDS, tm.LONGEST)
    assert (kmc.TRIM_INVERT, kmc.TRIM_PAIR_BOTH, kmc.TRIM_PAIR_EITHER, kmc.TRIM_PASS, kmc.TRIM_EMITTED) == (1, 2, 4, 1, 2)
    no, nb = C.c_uint64(7), C.c_uint64(7)
    assert L.kmc_trim(None, 1, 0, 0, 0, 0, 0, 0, None, None, 0, None, 0, None, None, 0, None, None, C.byref(no), C.byref(nb), None) == kmc.ERR_ARG
    assert (no.value, nb.value) == (0, 0)
    no, nb = C.c_uint64(7), C.c_uint64(7)
    assert L.kmc_trim_device(None, 1, 0, 0, 0, 0, 0, 0, None, None, 0, 0, None, None, None, None, None, C.byref(no), C.byref(nb), None) == kmc.ERR_ARG
    assert (no.value, nb.value) == (0, 0)
    s = kmc.TrimSummary.from_words(range(8))
    assert s.words() == list(range(8)) and s.emitted == 4 and s.to_text().startswith("reads\t0\nvalid_windows\t1\n")


def test_cli_argument_errors():
    run = lambda *a: subprocess.run([EXE, SAMPLE] + list(a), capture_output=True, text=True)
    assert run("--trim", SAMPLE).returncode == 2                                                # needs -k
    assert run("-k", "31", "--trim", SAMPLE, "--invert", "--trim-mode", "ends").returncode == 2
    assert run("-k", "31", "--trim", SAMPLE, "--invert").returncode == 2                        # (the default mode trims)
    assert run("-k", "31", "--trim", SAMPLE, "--paired", "both", "--paired", "either").returncode == 2
    assert run("-k", "31", "--trim", SAMPLE, "--paired", "neither").returncode == 2
    assert run("-k", "31", "--trim", SAMPLE, "--trim-mode", "most").returncode == 2
    assert run("-k", "31", "--trim", SAMPLE, "--strong-permille", "1001").returncode == 2
    assert run("-k", "31", "--min-strong", "3").returncode == 2                                 # a trim option without --trim
    for other in (["--correct", SAMPLE], ["--map", SAMPLE], ["--profile", SAMPLE], ["--query-kmers", SAMPLE]):
        assert run("-k", "31", "--trim", SAMPLE, *other).returncode == 2
