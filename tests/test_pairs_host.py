"""CPU checks of the pair model (tests/pair_model.py) that the GPU tests compare kmc_unitig_pairs against: the identities
include/kmc.h states hold on every input, every class and the tie rule occur, and the constructed inputs give the distances
they were built with, so a mistake in the model cannot hide behind an equal mistake in the library.  Also what needs no GPU
of the feature's surface: the ABI lists, the binding sources, the text form and the CLI's usage errors."""
import os
import re
import subprocess

import numpy as np
import pytest

import graph_model as gm
import pair_inputs as pi
import pair_model as pm
from conftest import ROOT, SAMPLE

KS = (5, 6, 31, 32, 33, 63)
RANGES = ((1, 0), (2, 0))


def _inputs(k):
    return [("library", pi.library(k, 700 + k)), ("gap", pi.gap(k, 710 + k, 120)), ("adjacent", pi.adjacent(k, 720 + k)),
            ("hot", pi.hot(k, 730 + k, 150)), ("edges", pi.edges(k, 740 + k)), ("small", pi.small(k, 760 + k))]


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", KS)
def test_identities_and_every_class(k, canonical):
    """Pairs.__init__ asserts the four identities; here every class and the tie rule must occur, at every k"""
    seen = {c: 0 for c in range(5)}
    ties = 0
    for name, (sample, pairs) in _inputs(k):
        table = gm.count_table(sample, k, canonical)
        for lo, hi in RANGES:
            p = pm.pairs(table, canonical, [pi.reads_of(pairs)], lo, hi)
            w = p.summary
            assert w[0] == len(pairs) == len(p.pair_class) and w[6] == len(p.rec_count), (name, k, canonical, lo, hi)
            assert all(lo_ <= hi_ and c * lo_ <= s <= c * hi_ for c, s, lo_, hi_ in zip(p.rec_count, p.rec_sum, p.rec_min, p.rec_max))
            assert p.rec_ends == sorted(p.rec_ends) and all(a < b for a, b in p.rec_ends)
            if (lo, hi) == (1, 0):
                for c in range(5):
                    seen[c] += w[1 + c]
                ties += p.ties
                if name == "edges":     # the special pairs sit at the seams, and each is what it was built as
                    for at in pi.EDGE_AT:
                        kind = pairs[at].kind
                        want = pi.EDGE_CLASS[kind] if canonical or kind in ("junk", "same") else pm.UNPLACED      # (forward: no reverse mate is placed)
                        assert p.pair_class[at] == want, (k, canonical, at, kind, p.pair_class[at])
                if name == "small":     # ... and so is every pair of the small graph, with the insert size it was cut with
                    for x, c, v in zip(pairs, p.pair_class, p.pair_value):
                        want = {"fr": pm.PROPER, "span": pm.SPAN, "ff": pm.SPAN, **pi.EDGE_CLASS}[x.kind]
                        if canonical:
                            assert c == want and (c != pm.PROPER or v == x.frag), (k, x, c, v)
                        elif x.kind in ("junk", "same", "ff"):
                            assert c == want, (k, x, c)
    # a forward ctx places no reverse mate: no pair there has o_A != o_B
    must = range(5) if canonical else (pm.UNPLACED, pm.SPAN, pm.SAME_STRAND)
    assert all(seen[c] > 0 for c in must) and ties > 0, (seen, ties)
    if not canonical:
        assert seen[pm.PROPER] == seen[pm.EVERTED] == 0


# The constructed truths below speak of places on a genome; they hold where a unitig names one place of it.  At k = 5 and 6
# a genome of a kilobase repeats its k-mers, its unitigs are a tangle of a few keys each, and "the end of the unitig" is no
# place on the genome -- so they are asserted for k >= 31, where random stretches are one unitig each.
@pytest.mark.parametrize("k", [31, 32, 33, 63])
def test_constructed_distances(k):
    # gap: F_true - R == g for every SPAN pair
    for g in (0, 1, 77, 300):
        sample, pairs = pi.gap(k, 710 + k, g)
        p = pm.pairs(gm.count_table(sample, k, True), True, [pi.reads_of(pairs)])
        assert p.summary[2] == len(pairs) and p.summary[6] == 1, (k, g, p.summary)
        assert all(x.frag - R == g for x, R in zip(pairs, p.pair_value))
        assert p.rec_count == [len(pairs)] and p.rec_sum == [sum(x.frag - g for x in pairs)]
    # adjacent: R - F_true == k - 1, so the estimated gap of a linked pair of ends is -(k - 1)
    sample, pairs = pi.adjacent(k, 720 + k)
    p = pm.pairs(gm.count_table(sample, k, True), True, [pi.reads_of(pairs)])
    assert p.summary[2] == len(pairs) and p.summary[6] == 1, (k, p.summary)
    assert all(R - x.frag == k - 1 for x, R in zip(pairs, p.pair_value))
    # library: every PROPER pair's F is the fragment length it was cut with
    sample, pairs = pi.library(k, 700 + k)
    p = pm.pairs(gm.count_table(sample, k, True), True, [pi.reads_of(pairs)])
    proper = [(x, F) for x, c, F in zip(pairs, p.pair_class, p.pair_value) if c == pm.PROPER]
    assert len(proper) >= 10 and all(x.kind in ("fr", "tie") and x.frag == F for x, F in proper), (k, len(proper))
    assert sum(p.hist) == len(proper) and all(p.hist[F] > 0 for _, F in proper)
    assert [c for x, c in zip(pairs, p.pair_class) if x.kind == "tie"] == [pm.PROPER]
    # the open last bin
    small = pm.pairs(gm.count_table(sample, k, True), True, [pi.reads_of(pairs)], n_bins=200)
    assert small.hist[199] == sum(1 for _, F in proper if F >= 199) > 0 and sum(small.hist) == len(proper)


@pytest.mark.parametrize("canonical", [True, False])
def test_concatenation_equals_accumulate_in_the_model(canonical):
    k = 31
    sample, pairs = pi.library(k, 700 + k)
    table = gm.count_table(sample, k, canonical)
    parts = [pairs[:37], [], pairs[37:38], pairs[38:]]
    whole = pm.pairs(table, canonical, [pi.reads_of(pairs)])
    acc = pm.pairs(table, canonical, [pi.reads_of(x) for x in parts])
    assert acc.totals() == whole.totals()
    assert acc.arrays()[:3] == pm.pairs(table, canonical, [pi.reads_of(parts[-1])]).arrays()[:3]      # the per-pair arrays: the last batch alone


def test_more_records_than_a_sort_leaf():
    k = 31
    sample, pairs = pi.many_records(k, 750)
    p = pm.pairs(gm.count_table(sample, k, True), True, [pi.reads_of(pairs)])
    assert p.summary[6] > 2048, p.summary


def _python_form(kmc, p):
    U64 = np.uint64
    return kmc.PairLinks(np.array(p.pair_class, np.uint8), np.array(p.pair_ends, np.uint32).reshape(-1, 2), np.array(p.pair_value, U64),
                         np.array(p.rec_ends, np.uint32).reshape(-1, 2), np.array(p.rec_count, U64), np.array(p.rec_sum, U64),
                         np.array(p.rec_min, U64), np.array(p.rec_max, U64), np.array(p.hist, U64), kmc.PairSummary.from_words(p.summary))


def test_python_pair_links_print_the_models_text(kmc):
    """PairLinks.to_text(), records(), insert_median() and gaps() on the model's arrays: no GPU is needed for them"""
    k = 31
    sample, pairs = pi.library(k, 700 + k)
    p = pm.pairs(gm.count_table(sample, k, True), True, [pi.reads_of(pairs)])
    r = _python_form(kmc, p)
    assert r.to_text() == p.text() and r.to_text().count("I\t") > 0 and r.to_text().count("P\t") == len(r) == p.summary[6] > 0
    assert [list(x[:2]) for x in r.records()] == p.rec_ends and [x[3] for x in r.records()] == p.rec_sum
    inserts = sorted(F for c, F in zip(p.pair_class, p.pair_value) if c == pm.PROPER)
    assert r.insert_median() == inserts[(len(inserts) - 1) // 2]
    sample, pairs = pi.adjacent(k, 720 + k)
    p = pm.pairs(gm.count_table(sample, k, True), True, [pi.reads_of(pairs)])
    r = _python_form(kmc, p)
    assert r.insert_median() is None and r.to_text() == p.text()
    mean = sum(x.frag for x in pairs) / len(pairs)
    assert list(r.gaps(mean)) == [-(k - 1)]                                  # two ends joined by a link
    assert _python_form(kmc, pm.pairs({}, True, [pi.reads_of(pairs)], k=k)).to_text() == ""


def test_abi_lists_hold_the_pair_calls(kmc):
    names = ("kmc_unitig_pairs", "kmc_unitig_pairs_device")
    assert all(n in kmc.ABI_SYMBOLS for n in names)
    with open(os.path.join(ROOT, "rust", "src", "lib.rs")) as f:
        rs = f.read()
    assert all(re.search(r"pub fn %s\(" % n, rs) for n in names) and "pub fn pairs(" in rs
    with open(os.path.join(ROOT, "include", "kmc.h")) as f:
        hdr = f.read()
    assert all(re.search(r"\bint %s\(" % n, hdr) for n in names)
    assert "#define KMC_PAIR_WORDS %d" % kmc.PAIR_WORDS in hdr and "#define KMC_PAIR_ACCUMULATE %du" % kmc.PAIR_ACCUMULATE in hdr
    for i, n in enumerate(("UNPLACED", "SPAN", "PROPER", "EVERTED", "SAME_STRAND")):
        assert "#define KMC_PAIR_%s %d" % (n, i) in hdr and getattr(kmc, "PAIR_" + n) == i == getattr(pm, n)
    with open(os.path.join(ROOT, "README.md")) as f:
        readme = f.read()
    assert "kmc_unitig_pairs" in readme and "measure_pairs.py" in readme and "--pairs" in readme
    assert all(hasattr(kmc.KmerCounter, n) for n in ("pair_links", "pair_links_device", "pair_links_tensors"))
    assert all(hasattr(kmc.PairLinks, n) for n in ("records", "insert_median", "gaps", "to_text"))
    assert kmc.PairSummary.from_words(range(8)).words() == list(range(8))
    assert [getattr(kmc.PairSummary.from_words(range(8)), f) for f in pm.FIELDS] == list(range(8))


def test_cli_rejects_pairs_without_k(kmc):
    exe = os.path.join(ROOT, "bin", "k-mer-count")
    for argv in (["--pairs", "x"], ["--pairs"], ["-k", "31", "--pairs", "x", "--gfa"], ["-k", "31", "--pairs", "x", "--map", "y"],
                 ["-k", "31", "--pairs", "x", "--transits", "y"], ["-k", "31", "--pairs", "x", "--histo", "5"], ["-k", "31", "--insert-bins", "200"],
                 ["-k", "31", "--pairs", "x", "--insert-bins", "z"], ["-k", "31", "--pairs", "x", "--insert-bins", "1"],
                 ["-k", "31", "--pairs", "x", "--insert-bins", "1048577"]):
        r = subprocess.run([exe, SAMPLE] + argv, capture_output=True, text=True)
        assert r.returncode == 2 and r.stdout == "" and "k-mer-count:" in r.stderr, (argv, r.returncode, r.stderr)
    r = subprocess.run([exe, SAMPLE, "--pairs", "x"], capture_output=True, text=True)
    assert "--pairs needs -k K" in r.stderr
