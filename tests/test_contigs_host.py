"""CPU checks of the contig model (tests/contig_model.py) that the GPU tests compare kmc_unitig_contigs against: the
identities include/kmc.h states are held on every input, and the constructed inputs must give the contigs they were built
for, so a mistake in the model cannot hide behind an equal mistake in the library.  Also what needs no GPU of the feature's
surface: the ABI lists, the binding sources, the FASTA and GFA text and the CLI's usage errors."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import contig_inputs as ci
import contig_model as cm
import graph_model as gm
import transit_inputs as ti
import transit_model as tm
import unitig_model as um
from conftest import ROOT, SAMPLE

NEVER = 1 << 63      # a min_reads no slot reaches: nothing is resolved


@functools.lru_cache(maxsize=None)
def _graph(name, k, canonical, lo=1, hi=0):
    """(the Case, the transit model, the unitig model) of an input: computed once, shared by the tests, never changed"""
    case = ci.make(name, k)
    table = gm.count_table(case.sample, k, canonical)
    return case, tm.transits(table, canonical, [case.reads], lo, hi, k=k), um.unitigs(table, canonical, lo, hi)


def _rotations(g):
    return {g[i:] + g[:i] for i in range(len(g))}


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("name,k", ci.cases())
def test_identities(name, k, canonical):
    for lo, hi in ((1, 0), (2, 0)):
        case, t, u = _graph(name, k, canonical, lo, hi)
        for min_reads, min_support in ((1, 0), (ti.PAIR_DEPTH, 0), (1, 1), (1, 2), (0, NEVER), (NEVER, 0)):
            c = cm.Contigs(t, u, min_reads, min_support)
            ctx = (name, k, canonical, lo, hi, min_reads, min_support)
            w = c.summary
            assert c.spelled_overlaps_agree, ctx
            used = [0] * len(u.seqs)
            for e in c.path:
                used[e >> 1] += 1
            assert used == c.copies, ctx                                          # every unitig as often as it has copies
            keys = sum(len(u.seqs[e >> 1]) - k + 1 for e in c.path)
            assert w[0] == len(c.seqs) == len(c.abund) == len(c.flags) and w[1] == c.path_offsets[-1] == len(c.path) == sum(c.copies), ctx
            assert w[7] == c.offsets[-1] == keys + w[0] * (k - 1), ctx
            assert all(len(s) == sum(len(u.seqs[e >> 1]) - k + 1 for e in p) + k - 1 for s, p in zip(c.seqs, c.paths())), ctx
            assert w[2] == sum(1 for x in c.copies if x > 1) and w[4] == sum(c.flags) and w[6] == max(map(len, c.paths()), default=0), ctx
            assert w[5] == sum(1 for p in c.paths() if len(p) == 1), ctx
            assert [p[0] for p in c.paths()] or not u.seqs, ctx
            starts = [c.node_offsets[p[0] >> 1] for p in c.paths()]
            assert min_support or w[3] == 0, ctx
            if w[2] == 0:
                assert starts == sorted(starts), ctx                              # numbered by their start node
            assert sum(c.abund) == sum(u.abund[e >> 1] for e in c.path), ctx


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("name,k", ci.cases())
def test_nothing_resolved_gives_the_unitigs(name, k, canonical):
    """min_reads = 2^63, min_support = 0: strings, offsets, abundances and flags of the unitig model, path[c] == [2c].  No input
    tried here breaks it, even-k canonical ones with palindromic keys included: a record that the unitigs refused to join
    over is refused by the mutual rule here for the same reason."""
    for lo, hi in ((1, 0), (2, 0)):
        case, t, u = _graph(name, k, canonical, lo, hi)
        c = cm.Contigs(t, u, NEVER, 0)
        assert c.seqs == u.seqs and c.offsets == u.offsets and c.abund == u.abund and c.flags == u.flags, (name, k, canonical, lo, hi)
        assert c.paths() == [[2 * i] for i in range(len(u.seqs))] and c.summary[2:4] == [0, 0]


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", ci.LONG_KS)
def test_constructed_inputs_give_their_contigs(k, canonical):
    for name in ci.SPELL_GENOMES:
        if k not in ci.INPUTS[name][1]:
            continue
        case, t, u = _graph(name, k, canonical)
        c = cm.Contigs(t, u)
        want = sorted(min(g, gm.revcomp(g)) for g in case.genomes)
        assert sorted(min(s, gm.revcomp(s)) for s in c.seqs) == want, (name, k, canonical, c.summary)
        assert c.summary[4] == 0 and c.summary[2] > 0
    # the shapes by number
    c = cm.Contigs(*_graph("repeat", k, canonical)[1:])
    assert c.summary[:3] == [2, 6, 1] and sorted(c.copies) == [1, 1, 1, 1, 2] and c.summary[6] == 3
    depth = ti.PAIR_DEPTH if canonical else ti.PAIR_DEPTH // 2
    assert cm.Contigs(*_graph("repeat", k, canonical)[1:], depth).summary[:3] == [2, 6, 1]
    assert cm.Contigs(*_graph("repeat", k, canonical)[1:], depth + 1).summary[:3] == [5, 5, 0]
    c = cm.Contigs(*_graph("tandem", k, canonical)[1:])
    assert c.summary[0] == 1 and c.summary[2] == 1 and max(c.copies) == 2
    walked = [e >> 1 for e in c.path]
    assert len(walked) == len(set(walked)) + 1                                    # the repeat's unitig is walked twice
    c = cm.Contigs(*_graph("two_repeats", k, canonical)[1:])
    assert c.summary[:3] == [2, 10, 2] and c.summary[6] == 5
    c = cm.Contigs(*_graph("ladder", k, canonical)[1:])
    assert c.summary[:3] == [66, 198, 33] and min(len(s) - k + 1 for s in _graph("ladder", k, canonical)[2].seqs) == 1
    # plasmids: two circular contigs, each its genome from some rotation on, with the first k - 1 bases once more
    case, t, u = _graph("plasmids", k, canonical)
    c = cm.Contigs(t, u)
    assert c.summary[0] == 2 and c.flags == [1, 1] and c.summary[4] == 2 and c.summary[2] == 1
    rot = [_rotations(g) | _rotations(gm.revcomp(g)) for g in case.genomes]
    hit = sorted(i for s in c.seqs for i, r in enumerate(rot) if len(s) == len(case.genomes[i]) + k - 1 and s[:len(case.genomes[i])] in r
                 and s[len(case.genomes[i]):] == s[:k - 1])
    assert hit == [0, 1]
    # nothing duplicated
    for name in ci.NOTHING_DUPLICATED:
        c = cm.Contigs(*_graph(name, k, canonical)[1:])
        assert c.summary[2] == 0 and c.summary[1] == len(c.copies), name
    if k % 2 == 1:
        case, t, u = _graph("hairpin", k, canonical)
        assert cm.Contigs(t, u).summary[0] == 1


@pytest.mark.parametrize("canonical", [True, False])
def test_chains_are_long_paths_and_cycles(canonical):
    k = 31
    case, t, u = _graph("chain", k, canonical)
    c = cm.Contigs(t, u)
    assert c.summary[:3] == [2, 522, 130] and c.summary[6] == 261 and c.summary[4] == 0
    case, t, u = _graph("chain_circular", k, canonical)
    c = cm.Contigs(t, u)
    assert c.summary[:3] == [2, 520, 130] and c.summary[6] == 260 and c.flags == [1, 1]
    for s in c.seqs:
        hit = [g for g in case.genomes if s[:len(g)] in _rotations(g) | _rotations(gm.revcomp(g))]
        assert len(hit) == 1 and len(s) == len(hit[0]) + k - 1
        assert s[:len(hit[0])] not in (hit[0], gm.revcomp(hit[0]))               # cut in the middle of the genome's own spelling


@pytest.mark.parametrize("k", [5, 6])
def test_support_threshold_cuts_links(k):
    """tangle: min_support ignores records, so joins appear (an end left with one live record) and disappear"""
    seen = set()
    for canonical in (True, False):
        case, t, u = _graph("tangle", k, canonical)
        for ms in (0, 1, 2):
            c = cm.Contigs(t, u, 1, ms)
            seen.add((c.summary[0], c.summary[3]))
            assert (c.summary[3] > 0) == (ms > 0 and any(x < ms for x in t.link_support))
    assert len(seen) >= 4


def test_text_is_fasta_with_walks():
    k = 31
    case, t, u = _graph("repeat", k, True)
    c = cm.Contigs(t, u)
    lines = c.text().splitlines()
    assert len(lines) == 4 and lines[1] == c.seqs[0] and lines[3] == c.seqs[1]
    assert re.fullmatch(r">0 LN:i:%d KC:i:%d CL:i:0 WK:Z:([<>]\d+){3}" % (len(c.seqs[0]), c.abund[0]), lines[0]), lines[0]
    assert cm.contigs({}, True, [case.reads], k=k).text() == "" and cm.contigs({}, True, [], k=k).summary == [0] * 8


def test_abi_lists_hold_the_contig_calls(kmc):
    names = ("kmc_unitig_contigs", "kmc_unitig_contigs_device")
    assert all(n in kmc.ABI_SYMBOLS for n in names)
    with open(os.path.join(ROOT, "rust", "src", "lib.rs")) as f:
        rs = f.read()
    assert all(re.search(r"pub fn %s\(" % n, rs) for n in names) and "pub fn contigs(" in rs
    with open(os.path.join(ROOT, "include", "kmc.h")) as f:
        hdr = f.read()
    assert "#define KMC_CONTIG_WORDS %d" % kmc.CONTIG_WORDS in hdr
    with open(os.path.join(ROOT, "README.md")) as f:
        readme = f.read()
    assert "kmc_unitig_contigs" in readme and "measure_contigs.py" in readme
    assert all(hasattr(kmc.KmerCounter, n) for n in ("contigs", "contigs_device"))
    assert all(hasattr(kmc.Contigs, n) for n in ("strings", "to_fasta", "paths", "walks", "to_text"))
    assert [getattr(kmc.ContigSummary.from_words(range(8)), f) for f in cm.FIELDS] == list(range(8))
    assert kmc.ContigSummary.from_words(range(8)).words() == list(range(8))


def _py(kmc, c):
    """the model's Contigs as the package's"""
    return kmc.Contigs(np.frombuffer(c.bases.encode(), np.uint8), np.array(c.offsets, np.uint64), np.array(c.path_offsets, np.uint64),
                       np.array(c.path, np.uint32), np.array(c.abund, np.uint64), np.array(c.flags, np.uint8), kmc.ContigSummary.from_words(c.summary))


def test_python_contigs_print_the_models_text(kmc):
    """Contigs.to_fasta() / walks() / paths() and to_gfa(links, k, contigs=) on the model's arrays: no GPU is needed to format them"""
    import links_model as lm
    k = 31
    for name in ("repeat", "plasmids"):
        case, t, u = _graph(name, k, True)
        c = cm.Contigs(t, u)
        pc = _py(kmc, c)
        assert pc.to_fasta() == pc.to_text() == c.text() and pc.strings() == c.seqs and pc.paths() == c.paths() and pc.walks() == c.walks()
        assert len(pc) == c.summary[0]
        lk = kmc.UnitigLinks(np.array(t.lk.offsets, np.uint64), np.array(t.lk.to, np.uint32), kmc.LinkSummary.from_words(t.lk.summary))
        offs = np.zeros(len(u.seqs) + 1, np.uint64)
        offs[1:] = np.cumsum([len(s) for s in u.seqs])
        un = kmc.Unitigs(np.frombuffer("".join(u.seqs).encode(), np.uint8), offs, np.array(u.abund, np.uint64), np.array(u.flags, np.uint8),
                         kmc.UnitigSummary.from_words(u.summary))
        old = lm.gfa(u, t.lk, k)
        assert un.to_gfa(lk, k) == old                                        # without the argument: byte for byte what it was
        new = un.to_gfa(lk, k, contigs=pc)
        assert new.startswith(old)
        p_lines = new[len(old):].splitlines()
        assert len(p_lines) == len(c.seqs)
        for i, (line, path, flag) in enumerate(zip(p_lines, c.paths(), c.flags)):
            f = line.split("\t")
            assert f[:2] == ["P", str(i)] and f[2] == ",".join("%d%s" % (e >> 1, "-" if e & 1 else "+") for e in path)
            assert f[3] == ",".join(["%dM" % (k - 1)] * (len(path) - 1 + flag))


@pytest.mark.parametrize("name,k", [("repeat", 31), ("tandem", 32), ("plasmids", 33), ("ladder", 63), ("chain_circular", 31), ("tangle", 5), ("tangle", 6)])
def test_the_measuring_tools_numpy_form_is_the_model(name, k):
    """tools/measure_contigs.host_contigs, the host baseline of the measurements, gives the model's arrays and words"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import measure_contigs as mc
    U64 = np.uint64
    for canonical in (True, False):
        case, t, u = _graph(name, k, canonical)
        for min_reads, min_support in ((1, 0), (1, 2), (NEVER, 0)):
            c = cm.Contigs(t, u, min_reads, min_support)
            got = mc.host_contigs(np.array(t.lk.offsets, U64), np.array(t.lk.to, np.uint32), np.array(t.link_support, U64), np.array(t.transit_offsets, U64),
                                  np.array(t.transit_count, U64), np.frombuffer("".join(u.seqs).encode(), np.uint8), np.array(u.offsets, U64),
                                  np.array(u.abund, U64), k, min_reads, min_support)
            want = (np.frombuffer(c.bases.encode(), np.uint8), np.array(c.offsets, U64), np.array(c.path_offsets, U64), np.array(c.path, np.uint32),
                    np.array(c.abund, U64), np.array(c.flags, np.uint8))
            assert all(np.array_equal(x, y) for x, y in zip(got[:6], want)) and got[6] == c.summary, (name, k, canonical, min_reads, min_support)


def test_cli_rejects_contigs_without_k(kmc):
    exe = os.path.join(ROOT, "bin", "k-mer-count")
    for argv in (["--contigs", "x"], ["--contigs"], ["-k", "31", "--contigs", "x", "--gfa"], ["-k", "31", "--contigs", "x", "--transits", "y"],
                 ["-k", "31", "--min-support", "2"], ["-k", "31", "--contigs", "x", "--min-support", "z"]):
        r = subprocess.run([exe, SAMPLE] + argv, capture_output=True, text=True)
        assert r.returncode == 2 and r.stdout == "" and "k-mer-count:" in r.stderr, (argv, r.returncode, r.stderr)
    r = subprocess.run([exe, SAMPLE, "--contigs", "x"], capture_output=True, text=True)
    assert "--contigs needs -k K" in r.stderr
