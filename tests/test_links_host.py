"""CPU-side checks of the unitig links: the two entry points are exported and keep their argument rules without a device,
the header section, the CLI knows --gfa and rejects bad uses of it before touching a GPU, LinkSummary / UnitigLinks /
Unitigs.to_gfa, and the Python model the GPU tests compare against (tests/links_model.py): hand-worked answers for tiny
inputs, the degree identity, and an independent brute force over the spelled unitig strings."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import graph_model as gm
import links_model as lm
import unitig_model as um
from conftest import ROOT, SAMPLE
from test_unitig_host import _random_reads

NEW = ("kmc_unitig_links", "kmc_unitig_links_device")
EXE = os.path.join(ROOT, "bin", "k-mer-count")


def test_library_exports_the_link_calls(kmc):
    out = subprocess.run(["nm", "-D", "--defined-only", kmc.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for s in NEW:
        assert f" T {s}\n" in out, s
        assert s in kmc.ABI_SYMBOLS
    L = kmc.lib()
    a = np.full(8, 7, np.uint64)
    p = a.ctypes.data
    n1, n2 = C.c_uint64(7), C.c_uint64(7)
    # a NULL ctx: KMC_ERR_ARG, the sizes zeroed, nothing written
    assert L.kmc_unitig_links(None, 1, 0, p, 4, p, 4, C.byref(n1), C.byref(n2), p) == kmc.ERR_ARG
    assert n1.value == 0 and n2.value == 0 and (a == 7).all()
    assert L.kmc_unitig_links(None, 1, 0, None, 0, None, 0, None, None, None) == kmc.ERR_ARG
    assert L.kmc_unitig_links_device(None, 1, 0, None, None, None, None, None) == kmc.ERR_ARG
    assert kmc.LINK_WORDS == 8 == len(lm.FIELDS)


def test_header_declares_the_link_section():
    hdr = open(os.path.join(ROOT, "include", "kmc.h")).read()
    assert "#define KMC_LINK_WORDS 8" in hdr
    assert "cap_ends counts ENDS" in hdr and "A links call counts as a kmc_unitigs* call" in hdr
    assert "kmc_unitig_links / kmc_unitig_links_device" in hdr.split("Conventions")[0]     # the mapping table at the top


@pytest.mark.parametrize("argv", [
    ["--gfa"],                                                                           # without -k
    ["-k", "5", "--gfa", "--graph"], ["-k", "5", "--gfa", "--graph-stats"], ["-k", "5", "--gfa", "--unitigs"],
    ["-k", "5", "--gfa", "--histo", "10"], ["-k", "5", "--gfa", "--query-kmers", "KMERS"],
    ["-k", "5", "--gfa", "--profile", "SAMPLE"], ["-k", "5", "--gfa", "--with", "SAMPLE", "--compare"],
    ["-k", "5", "--gfa", "--with", "SAMPLE", "--setop", "union"], ["-k", "5", "--gfa", "--with", "SAMPLE"],
    ["-k", "5", "--gfa", "--compare"], ["-k", "5", "--gfa", "--setop", "union"], ["-k", "5", "--gfa", "--expand"],
    ["-k", "5", "--gfa", "--min-count", "3", "--max-count", "2"]])
def test_cli_rejects_bad_gfa_options(kmc, tmp_path, argv):
    kmers = tmp_path / "kmers.txt"
    kmers.write_text("ACGTA\n")
    argv = [SAMPLE if a == "SAMPLE" else str(kmers) if a == "KMERS" else a for a in argv]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")   # no GPU to touch even where there is one
    r = subprocess.run([EXE, SAMPLE] + argv, capture_output=True, text=True, env=env)
    assert r.returncode == 2 and r.stdout == "" and "k-mer-count:" in r.stderr, (argv, r.returncode, r.stderr)
    assert "unknown option" not in r.stderr, r.stderr      # rejected as a known option in a bad combination


def test_cli_help_lists_gfa(kmc):
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == ""
    assert "--gfa" in r.stderr and "--graph | --graph-stats | --unitigs | --gfa" in r.stderr


# the SNP bubble of the hand-written cases: ACA forks into CAG-AGG-GGT and CAT-ATG-TGT, which meet again in GTC
_BUBBLE = ["ACAGGTC", "ACATGTC"]


@pytest.mark.parametrize("reads,k,canonical,seqs,offsets,to,words", [
    # one linear read: one unitig, both ends bare
    (["ACGTT"], 3, False, ["ACGTT"], [0, 0, 0], [], [1, 0, 2, 0, 0, 0, 1, 0]),
    (["ACGGT"], 4, False, ["ACGGT"], [0, 0, 0], [], [1, 0, 2, 0, 0, 0, 1, 0]),
    # the fork AAC -> ACG / ACT: the END end of AAC reaches both START ends (ascending base: G, T), each reaches back
    (["AACG", "AACT"], 3, False, ["AAC", "ACG", "ACT"], [0, 0, 2, 3, 3, 4, 4], [2, 4, 1, 1], [3, 4, 3, 1, 0, 0, 0, 2]),
    # the bubble: four unitigs ACA, CAGGT, CATGT, GTC; two records at the fork, two at the merge, one at each branch end
    (_BUBBLE, 3, False, ["ACA", "CAGGT", "CATGT", "GTC"], [0, 0, 2, 3, 4, 5, 6, 8, 8], [2, 4, 1, 6, 1, 6, 3, 5], [4, 8, 2, 2, 0, 0, 0, 2]),
    # a homopolymer: a circular one-key unitig, END -> START and its mirror
    (["AAAAA"], 3, False, ["AAA"], [0, 1, 2], [1, 0], [1, 2, 0, 0, 2, 0, 0, 1]),
    (["AAAAA"], 3, True, ["AAA"], [0, 1, 2], [1, 0], [1, 2, 0, 0, 2, 0, 0, 1]),
    (["AAAAAA"], 4, True, ["AAAA"], [0, 1, 2], [1, 0], [1, 2, 0, 0, 2, 0, 0, 1]),
    # a cycle of three keys, cut: END -> START of the same unitig
    (["ACGACG"], 3, False, ["ACGAC"], [0, 1, 2], [1, 0], [1, 2, 0, 0, 2, 0, 0, 1]),
    # a hairpin: ACG + T = CGT = revcomp(ACG): the END end is linked to itself, once
    (["ACGT"], 3, True, ["ACG"], [0, 0, 1], [1], [1, 1, 1, 0, 1, 0, 0, 1]),
    # even k, the palindrome ACGT beside CGTC: side L of ACGT reaches side L of CGTC, which is joined to side R of ACGT
    (["GACGTC"], 4, True, ["ACGTC"], [0, 0, 0], [], [1, 0, 2, 0, 0, 1, 1, 0]),
    # nothing at all
    ([], 3, False, [], [0], [], [0] * 8),
])
def test_model_against_hand_written_answers(reads, k, canonical, seqs, offsets, to, words):
    table = gm.count_table(reads, k, canonical)
    assert um.unitigs(table, canonical).seqs == seqs
    lk = lm.links(table, canonical)
    assert (lk.offsets, lk.to, lk.summary) == (offsets, to, words)


def test_model_records_in_gfa_terms():
    table = gm.count_table(_BUBBLE, 3, False)
    lk = lm.links(table, False)
    assert list(lk.records()) == [(0, "+", 1, "+"), (0, "+", 2, "+"), (1, "-", 0, "-"), (1, "+", 3, "+"), (2, "-", 0, "-"),
                                  (2, "+", 3, "+"), (3, "-", 1, "-"), (3, "-", 2, "-")]
    assert lm.gfa(um.unitigs(table, False), lk, 3) == (
        "H\tVN:Z:1.0\nS\t0\tACA\tLN:i:3\tKC:i:2\tCL:i:0\nS\t1\tCAGGT\tLN:i:5\tKC:i:3\tCL:i:0\nS\t2\tCATGT\tLN:i:5\tKC:i:3\tCL:i:0\n"
        "S\t3\tGTC\tLN:i:3\tKC:i:2\tCL:i:0\nL\t0\t+\t1\t+\t2M\nL\t0\t+\t2\t+\t2M\nL\t1\t-\t0\t-\t2M\nL\t1\t+\t3\t+\t2M\nL\t2\t-\t0\t-\t2M\n"
        "L\t2\t+\t3\t+\t2M\nL\t3\t-\t1\t-\t2M\nL\t3\t-\t2\t-\t2M\n")
    hp = lm.links(gm.count_table(["ACGT"], 3, True), True)
    assert list(hp.records()) == [(0, "+", 0, "-")]


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 7, 8, 21])
def test_model_properties_on_random_reads(k):
    rng = np.random.default_rng(2000 + k)
    dropped = 0
    for canonical in (True, False):
        for trial in range(3):
            table = gm.count_table(_random_reads(rng, k), k, canonical)
            for lo, hi in ((1, 0), (2, 0), (1, 1), (2, 3)):
                u = um.unitigs(table, canonical, lo, hi)
                lk = lm.links(table, canonical, lo, hi)
                g, t, w = gm.graph(table, canonical, lo, hi)[2], u.summary, lk.summary
                ctx = (k, canonical, trial, lo, hi)
                # the degree identity: every side that is not a unitig end has degree 1
                assert g[1] + g[2] == w[1] + w[5] + 2 * (t[2] - t[0]), ctx
                # the summary words agree with the records
                per_end = np.diff(lk.offsets) if len(lk.offsets) > 1 else np.zeros(0, int)
                assert lk.offsets[0] == 0 and lk.offsets[-1] == len(lk.to) == w[1] and len(lk.offsets) == 2 * t[0] + 1 and w[0] == t[0]
                assert w[2] == int((per_end == 0).sum()) and w[3] == int((per_end >= 2).sum()) and w[7] == int(per_end.max(initial=0)) <= 4
                assert w[4] == sum(1 for a, _, b, _ in lk.records() if a == b)
                assert w[6] == sum(1 for x in range(t[0]) if per_end[2 * x] == 0 and per_end[2 * x + 1] == 0)
                assert all(0 <= x < 2 * t[0] for x in lk.to)
                # the overlaps the records claim
                for a, o1, b, o2 in lk.records():
                    sa = u.seqs[a] if o1 == "+" else gm.revcomp(u.seqs[a])
                    sb = u.seqs[b] if o2 == "+" else gm.revcomp(u.seqs[b])
                    assert sa[len(sa) - (k - 1):] == sb[:k - 1], ctx
                    if not canonical:
                        assert (o1, o2) in (("+", "+"), ("-", "-")), ctx
                if not canonical or k % 2:
                    assert w[5] == 0, ctx
                    assert lm.brute_force(u.seqs, k, canonical) == (lk.offsets, lk.to), ctx
                    # every link from both of its ends: the record multiset is symmetric
                    pairs = sorted((2 * a + (o1 == "+"), 2 * b + (o2 == "-")) for a, o1, b, o2 in lk.records())
                    assert pairs == sorted((y, x) for x, y in pairs), ctx
                dropped += w[5]
    if k % 2 == 0 and k >= 4:   # (the reads nearly fill the space of 2-mers: nothing is joined there, so nothing is dropped)
        assert dropped > 0      # the palindrome read does what it is there for


def test_link_summary_and_result_objects(kmc):
    w = [4, 8, 2, 2, 0, 0, 0, 2]
    s = kmc.LinkSummary.from_words(np.array(w, np.uint64))
    assert s.words() == w and all(type(x) is int for x in s.words())
    assert (s.unitigs, s.records, s.ends_without, s.ends_branching, s.self_records, s.dropped, s.isolated_unitigs, s.max_records) == tuple(w)
    assert s.to_text() == "".join("%s\t%d\n" % (f, v) for f, v in zip(lm.FIELDS, w))
    table = gm.count_table(_BUBBLE, 3, False)
    u, lk = um.unitigs(table, False), lm.links(table, False)
    r = kmc.UnitigLinks(np.array(lk.offsets, np.uint64), np.array(lk.to, np.uint32), kmc.LinkSummary.from_words(lk.summary))
    assert len(r) == 8 and list(r.records()) == list(lk.records())
    assert all(type(x) is int for rec in r.records() for x in (rec[0], rec[2]))
    ru = kmc.Unitigs(np.frombuffer(u.bases.encode(), np.uint8), np.array(u.offsets, np.uint64), np.array(u.abund, np.uint64),
                     np.array(u.flags, np.uint8), kmc.UnitigSummary.from_words(u.summary))
    assert ru.to_gfa(r, 3) == lm.gfa(u, lk, 3)
    with pytest.raises(ValueError):
        ru.to_gfa(kmc.UnitigLinks(np.zeros(1, np.uint64), np.zeros(0, np.uint32), kmc.LinkSummary.from_words([0] * 8)), 3)
