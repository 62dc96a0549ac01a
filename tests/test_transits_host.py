"""CPU checks of the transit model (tests/transit_model.py) that the GPU tests compare kmc_unitig_transits against: the
identities include/kmc.h states are held on every input, and the constructed inputs must give the verdicts they were built
for, so a mistake in the model cannot hide behind an equal mistake in the library.  Also what needs no GPU of the feature's
surface: the ABI lists, the binding sources, the GFA text and the CLI's usage errors."""
import os
import re
import subprocess

import pytest

import graph_model as gm
import links_model as lm
import map_inputs as mi
import transit_inputs as ti
import transit_model as tm
import unitig_model as um
from conftest import ROOT, SAMPLE

KS = (5, 6, 31, 32, 33, 63)


def _inputs(k, canonical):
    out = [("repeat", ti.repeat(k, 500 + k)), ("short", ti.short(k, 500 + k)), ("chimera", ti.chimera(k, 500 + k)),
           ("genome", mi.genome_reads(k, 100 + k, n_reads=60, genome=1200)), ("circular", mi.circular(k, 200 + k))]
    if k == 31:
        out += [("two_graphs", mi.two_graphs(k, 300 + k, n_reads=10)), ("boundary", ti.read_boundary(k, 600, pairs=40))]
    if canonical and k % 2 == 1:
        out.append(("hairpin", mi.hairpin(k, 400 + k)))
    return out


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", KS)
def test_identities(k, canonical):
    seen = {"crossings": 0, "transits": 0, "dropped": 0, "loops": 0, "repeats": 0}
    for name, (sample, reads) in _inputs(k, canonical):
        table = gm.count_table(sample, k, canonical)
        for lo, hi in ((1, 0), (2, 0)):
            t = tm.transits(table, canonical, [reads], lo, hi)
            ctx = (name, k, canonical, lo, hi)
            w, m, lk = t.summary, t.maps[0], t.lk
            assert w[0] == m.summary[4], ctx                                     # [0] is the map call's crossings
            assert sum(t.transit_count) == w[3], ctx
            assert len(t.link_support) == lk.summary[1] and len(t.verdict) == len(t.seqs) == lk.summary[0], ctx
            assert w[2] == t.link_support.count(0) and w[5] == w[6] + w[7] + t.verdict.count(tm.UNSPANNED), ctx
            symmetric = all(t.record(x, e) is not None for e in range(len(lk.offsets) - 1) for x in lk.to[lk.offsets[e]:lk.offsets[e + 1]])
            if not canonical or k % 2 == 1:
                assert symmetric and lk.summary[5] == 0, ctx
            # (links summary [5] == 0 alone does not make an even-k canonical set symmetric: a palindromic key that is a
            # unitig of its own has both sides terminal, lists a neighbour at both, and is entered by it through one)
            if symmetric:
                assert w[1] == 0 and w[4] == 0, ctx
                assert sum(t.link_support) == 2 * w[0] - t.loops, ctx
            for _, s in t.transit_segments:                                      # a transit spans its whole unitig
                assert s[1] == len(t.seqs[s[2] >> 1]) - k + 1, (ctx, s)
            assert len(t.transit_segments) == w[3]
            for u in range(len(t.seqs)):
                assert len(t.matrix(u)) == t.d_start[u] and all(len(r) == t.d_end[u] for r in t.matrix(u))
            seen["crossings"] += w[0]; seen["transits"] += w[3]; seen["dropped"] += w[4]; seen["loops"] += t.loops; seen["repeats"] += w[5]
    assert seen["crossings"] > 0 and seen["transits"] > 0 and seen["repeats"] > 0, seen
    if canonical and k % 2 == 1:
        assert seen["loops"] > 0, seen                                           # the hairpin: a == b
    if canonical and k == 6:
        assert seen["dropped"] > 0, seen                                         # around palindromic keys a record is missing


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [31, 32, 33, 63])
def test_constructed_inputs_give_their_verdicts(k, canonical):
    depth = ti.PAIR_DEPTH if canonical else ti.PAIR_DEPTH // 2
    for name, want in (("repeat", tm.RESOLVED), ("short", tm.UNSPANNED), ("chimera", tm.AMBIGUOUS)):
        sample, reads = getattr(ti, name)(k, 500 + k)
        table = gm.count_table(sample, k, canonical)
        t = tm.transits(table, canonical, [reads])
        assert sorted(t.verdict) == sorted([tm.PLAIN] * 4 + [want]), (name, t.verdict)
        u = t.verdict.index(want)
        assert (t.d_start[u], t.d_end[u]) == (2, 2) and len(t.seqs[u]) == k + 12
        mat = t.matrix(u)
        if name == "repeat":
            assert sorted(map(sorted, mat)) == [[0, depth], [0, depth]] and mat[0][0] == mat[1][1], mat   # a 2 x 2 permutation
            assert t.summary == [4 * depth, 0, 0, 2 * depth, 0, 1, 1, 0] and set(t.link_support) == {depth}
            assert tm.transits(table, canonical, [reads], min_reads=depth).verdict[u] == tm.RESOLVED
            assert tm.transits(table, canonical, [reads], min_reads=depth + 1).verdict[u] == tm.UNSPANNED
            assert tm.transits(table, canonical, [reads], min_reads=0).verdict == t.verdict
            # batches add up
            parts = tm.transits(table, canonical, [reads[:7], [], reads[7:]])
            assert parts.arrays() == t.arrays() and parts.summary == t.summary
        elif name == "short":
            assert not any(map(any, mat)) and t.summary[0] > 0 and t.summary[3] == 0
        else:
            assert sorted(x for row in mat for x in row) == [0, depth, depth, depth], mat


def test_a_read_boundary_is_no_crossing():
    k = 31
    sample, reads = ti.read_boundary(k, 600)
    table = gm.count_table(sample, k, True)
    t = tm.transits(table, True, [reads])
    m = t.maps[0]
    firsts = [m.segments[m.seg_offsets[r]] for r in range(len(reads)) if m.seg_offsets[r + 1] > m.seg_offsets[r]]
    prevs = [m.segments[m.seg_offsets[r] - 1] for r in range(1, len(reads)) if m.seg_offsets[r + 1] > m.seg_offsets[r]]
    fake = [i for i, (f, p) in enumerate(zip(firsts[1:], prevs)) if f[0] == p[0] + p[1]]
    assert len(fake) >= 200                                              # what a lane that tests `start` alone would count
    at = {m.seg_offsets[r] for r in range(len(reads)) if m.seg_offsets[r + 1] > m.seg_offsets[r] and m.seg_offsets[r] > 0
          and m.segments[m.seg_offsets[r]][0] == 20}
    assert {64, 128, 192, 256} <= at and any(x % 64 for x in at)         # across a wave's edge, a workgroup's, inside a wave
    assert t.summary[0] == m.summary[4] == 4 * ti.PAIR_DEPTH


def test_text_lists_supported_records_and_repeats():
    k = 31
    sample, reads = ti.chimera(k, 1)
    t = tm.transits(gm.count_table(sample, k, True), True, [reads])
    lines = t.text().splitlines()
    assert [x[0] for x in lines] == ["L"] * 8 + ["U"] + ["T"] * 3 and lines[8].split("\t")[2:] == ["ambiguous", "2", "2"]
    assert sum(int(x.split("\t")[3]) for x in lines[:8]) == sum(t.link_support)
    assert tm.transits({}, True, [reads], k=k).text() == "" and tm.transits({}, True, [reads], k=k).transit_offsets == [0]


def test_abi_lists_hold_the_transit_calls(kmc):
    names = ("kmc_unitig_transits", "kmc_unitig_transits_device")
    assert all(n in kmc.ABI_SYMBOLS for n in names)
    with open(os.path.join(ROOT, "rust", "src", "lib.rs")) as f:
        rs = f.read()
    assert all(re.search(r"pub fn %s\(" % n, rs) for n in names) and "pub fn transits(" in rs
    with open(os.path.join(ROOT, "include", "kmc.h")) as f:
        hdr = f.read()
    assert "#define KMC_TRANSIT_WORDS %d" % kmc.TRANSIT_WORDS in hdr and "#define KMC_TRANSIT_ACCUMULATE %du" % kmc.TRANSIT_ACCUMULATE in hdr
    for i, n in enumerate(("PLAIN", "UNSPANNED", "RESOLVED", "AMBIGUOUS")):
        assert "#define KMC_TRANSIT_%s %d" % (n, i) in hdr and getattr(kmc, "TRANSIT_" + n) == i == getattr(tm, n)
    with open(os.path.join(ROOT, "README.md")) as f:
        readme = f.read()
    assert "kmc_unitig_transits" in readme and "measure_transits.py" in readme
    assert all(hasattr(kmc.KmerCounter, n) for n in ("transits", "transits_device", "transits_tensors"))
    assert all(hasattr(kmc.Transits, n) for n in ("matrix", "records", "to_text"))
    assert kmc.TransitSummary.from_words(range(8)).words() == list(range(8))
    assert [getattr(kmc.TransitSummary.from_words(range(8)), f) for f in tm.FIELDS] == list(range(8))


def test_python_transits_print_the_models_text(kmc):
    """Transits.to_text() and to_gfa(links, k, transits) on the model's arrays: no GPU is needed to format them"""
    import numpy as np
    k = 31
    sample, reads = ti.chimera(k, 1)
    table = gm.count_table(sample, k, True)
    t = tm.transits(table, True, [reads])
    u = um.unitigs(table, True)
    lk = kmc.UnitigLinks(np.array(t.lk.offsets, np.uint64), np.array(t.lk.to, np.uint32), kmc.LinkSummary.from_words(t.lk.summary))
    tr = kmc.Transits(np.array(t.link_support, np.uint64), np.array(t.transit_offsets, np.uint64), np.array(t.transit_count, np.uint64),
                      np.array(t.verdict, np.uint8), kmc.TransitSummary.from_words(t.summary), lk)
    assert tr.to_text() == t.text()
    assert [list(map(int, row)) for row in tr.matrix(t.verdict.index(tm.AMBIGUOUS))] == t.matrix(t.verdict.index(tm.AMBIGUOUS))
    assert [(e, to, s) for e, to, s in tr.records()] == [(e, t.lk.to[j], t.link_support[j]) for e in range(len(t.lk.offsets) - 1)
                                                         for j in range(t.lk.offsets[e], t.lk.offsets[e + 1])]
    bases = np.frombuffer("".join(u.seqs).encode(), np.uint8)
    offs = np.zeros(len(u.seqs) + 1, np.uint64)
    offs[1:] = np.cumsum([len(s) for s in u.seqs])
    un = kmc.Unitigs(bases, offs, np.array(u.abund, np.uint64), np.array(u.flags, np.uint8), kmc.UnitigSummary.from_words(u.summary))
    old = lm.gfa(u, t.lk, k)
    assert un.to_gfa(lk, k) == old                                       # without the argument: byte for byte what it was
    new = un.to_gfa(lk, k, tr).splitlines()
    want = old.splitlines()
    links = [i for i, x in enumerate(want) if x.startswith("L\t")]
    assert len(new) == len(want) and len(links) == len(t.link_support)
    for j, i in enumerate(links):
        assert new[i] == want[i] + "\tRC:i:%d" % t.link_support[j]
    assert all(new[i] == want[i] for i in range(len(want)) if i not in links)


def test_cli_rejects_transits_without_k(kmc):
    exe = os.path.join(ROOT, "bin", "k-mer-count")
    for argv in (["--transits", "x"], ["--transits"], ["-k", "31", "--transits", "x", "--gfa"], ["-k", "31", "--transits", "x", "--map", "y"],
                 ["-k", "31", "--transits", "x", "--histo", "5"], ["-k", "31", "--min-reads", "2"], ["-k", "31", "--transits", "x", "--min-reads", "z"]):
        r = subprocess.run([exe, SAMPLE] + argv, capture_output=True, text=True)
        assert r.returncode == 2 and r.stdout == "" and "k-mer-count:" in r.stderr, (argv, r.returncode, r.stderr)
    r = subprocess.run([exe, SAMPLE, "--transits", "x"], capture_output=True, text=True)
    assert "--transits needs -k K" in r.stderr
