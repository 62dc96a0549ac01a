"""CPU-side checks of the unitig feature: the two entry points are exported and reject a NULL ctx, the header macros, the
CLI rejects bad uses of --unitigs before touching a GPU, UnitigSummary's text, and the Python model the GPU tests compare
against (tests/unitig_model.py): hand-worked answers for tiny inputs and properties on random reads."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import graph_model as gm
import unitig_model as um
from conftest import ROOT, SAMPLE

NEW = ("kmc_unitigs", "kmc_unitigs_device")
EXE = os.path.join(ROOT, "bin", "k-mer-count")


def test_library_exports_the_unitig_calls(kmc):
    out = subprocess.run(["nm", "-D", "--defined-only", kmc.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for s in NEW:
        assert f" T {s}\n" in out, s
        assert s in kmc.ABI_SYMBOLS
    L = kmc.lib()
    a = np.full(8, 7, np.uint64)
    p = a.ctypes.data
    n1, n2 = C.c_uint64(7), C.c_uint64(7)
    assert L.kmc_unitigs(None, 1, 0, p, 4, p, p, p, 4, C.byref(n1), C.byref(n2), p) == kmc.ERR_ARG
    assert n1.value == 0 and n2.value == 0 and (a == 7).all()
    assert L.kmc_unitigs(None, 1, 0, None, 0, None, None, None, 0, None, None, None) == kmc.ERR_ARG
    assert L.kmc_unitigs_device(None, 1, 0, None, None, None, None, None, None, None) == kmc.ERR_ARG
    assert kmc.UNITIG_WORDS == 8 == len(um.FIELDS) and kmc.UNITIG_CIRCULAR == 1


def test_header_declares_the_unitig_section():
    hdr = open(os.path.join(ROOT, "include", "kmc.h")).read()
    assert "#define KMC_UNITIG_WORDS 8" in hdr and "#define KMC_UNITIG_CIRCULAR 1u" in hdr
    assert "kmc_unitigs* counts as a kmc_graph*" in hdr


@pytest.mark.parametrize("argv", [
    ["--unitigs"],                                                                       # without -k
    ["-k", "5", "--unitigs", "--graph"], ["-k", "5", "--unitigs", "--graph-stats"],
    ["-k", "5", "--unitigs", "--histo", "10"], ["-k", "5", "--unitigs", "--query-kmers", "KMERS"],
    ["-k", "5", "--unitigs", "--profile", "SAMPLE"], ["-k", "5", "--unitigs", "--with", "SAMPLE", "--compare"],
    ["-k", "5", "--unitigs", "--with", "SAMPLE", "--setop", "union"], ["-k", "5", "--unitigs", "--with", "SAMPLE"],
    ["-k", "5", "--unitigs", "--compare"], ["-k", "5", "--unitigs", "--setop", "union"], ["-k", "5", "--unitigs", "--expand"],
    ["-k", "5", "--unitigs", "--min-count", "3", "--max-count", "2"]])                    # an empty range, as everywhere
def test_cli_rejects_bad_unitig_options(kmc, tmp_path, argv):
    kmers = tmp_path / "kmers.txt"
    kmers.write_text("ACGTA\n")
    argv = [SAMPLE if a == "SAMPLE" else str(kmers) if a == "KMERS" else a for a in argv]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")   # no GPU to touch even where there is one
    r = subprocess.run([EXE, SAMPLE] + argv, capture_output=True, text=True, env=env)
    assert r.returncode == 2 and r.stdout == "" and "k-mer-count:" in r.stderr, (argv, r.returncode, r.stderr)
    assert "unknown option" not in r.stderr, r.stderr      # rejected as a known option in a bad combination


def test_cli_help_lists_unitigs(kmc):
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == ""
    assert "--graph | --graph-stats | --unitigs" in r.stderr


def test_unitig_summary_and_result_text(kmc):
    w = [3, 9, 3, 1, 3, 1, 2, 4]
    s = kmc.UnitigSummary.from_words(np.array(w, np.uint64))
    assert s.words() == w and all(type(x) is int for x in s.words())
    assert (s.unitigs, s.bases, s.keys, s.circular, s.one_key, s.longest_keys, s.unjoined_sides, s.abundance) == tuple(w)
    assert s.mean_keys == 1.0 and kmc.UnitigSummary.from_words([0] * 8).mean_keys == 0.0
    assert s.to_text() == "".join("%s\t%d\n" % (f, v) for f, v in zip(um.FIELDS, w))
    u = um.unitigs(gm.count_table(["AACG", "AACT", "TTTTT"], 3, False), False)
    r = kmc.Unitigs(np.frombuffer(u.bases.encode(), np.uint8), np.array(u.offsets, np.uint64), np.array(u.abund, np.uint64),
                    np.array(u.flags, np.uint8), kmc.UnitigSummary.from_words(u.summary))
    assert len(r) == 4 and r.strings() == u.seqs == ["AAC", "ACG", "ACT", "TTT"]
    assert r.to_fasta() == u.fasta() == (">0 LN:i:3 KC:i:2 CL:i:0\nAAC\n>1 LN:i:3 KC:i:1 CL:i:0\nACG\n>2 LN:i:3 KC:i:1 CL:i:0\nACT\n"
                                         ">3 LN:i:3 KC:i:3 CL:i:1\nTTT\n")


@pytest.mark.parametrize("reads,k,canonical,rng,seqs,abund,flags,words", [
    # ACG -> CGT -> GTT: one path, read from its smallest (and leftmost) key
    (["ACGTT"], 3, False, (1, 0), ["ACGTT"], [3], [0], [1, 5, 3, 0, 0, 3, 0, 3]),
    # forward: the reading leaves keys through R, whatever the rows of the end keys (TTG is the larger row)
    (["TTGCA"], 3, False, (1, 0), ["TTGCA"], [3], [0], [1, 5, 3, 0, 0, 3, 0, 3]),
    # the fork AAC -> ACG / ACT: three unitigs of one key
    (["AACG", "AACT"], 3, False, (1, 0), ["AAC", "ACG", "ACT"], [2, 1, 1], [0, 0, 0], [3, 9, 3, 0, 3, 1, 0, 4]),
    (["AACG", "AACT"], 3, False, (2, 0), ["AAC"], [2], [0], [1, 3, 1, 0, 1, 1, 0, 2]),
    # a key joined to itself: a cycle of one key, cut, spelled as stored
    (["AAAAA"], 3, False, (1, 0), ["AAA"], [3], [1], [1, 3, 1, 1, 1, 1, 0, 3]),
    (["AAAAA"], 3, True, (1, 0), ["AAA"], [3], [1], [1, 3, 1, 1, 1, 1, 0, 3]),
    # a cycle of three keys (ACG -> CGA -> GAC -> ACG), cut on the L side of ACG and spelled linearly from there
    (["ACGACG"], 3, False, (1, 0), ["ACGAC"], [4], [1], [1, 5, 3, 1, 0, 3, 0, 4]),
    # canonical: CAAG holds CAA and AAG.  AAG is the smaller row; its terminal side is R, so it is left through L: its
    # reverse complement CTT, then the last character of TTG
    (["CAAG"], 3, True, (1, 0), ["CTTG"], [2], [0], [1, 4, 2, 0, 0, 2, 0, 2]),
    # an AT repeat, odd k, canonical: either extension of ATATA is its own reverse complement, entered on the same side
    (["ATATATAT"], 5, True, (1, 0), ["ATATA"], [4], [0], [1, 5, 1, 0, 1, 1, 2, 4]),
    # a hairpin: ACG + T = CGT = revcomp(ACG): side R of ACG is its own partner
    (["ACGT"], 3, True, (1, 0), ["ACG"], [2], [0], [1, 3, 1, 0, 1, 1, 1, 2]),
    # even k, the palindrome ACGT between GACG and CGTC (one key, CGTC): both sides of ACGT name side L of CGTC, which
    # names side R of ACGT back
    (["GACGTC"], 4, True, (1, 0), ["ACGTC"], [3], [0], [1, 5, 2, 0, 0, 2, 1, 3]),
    # nothing solid
    (["ACGTT"], 3, False, (2, 0), [], [], [], [0] * 8),
])
def test_model_against_hand_written_answers(reads, k, canonical, rng, seqs, abund, flags, words):
    u = um.unitigs(gm.count_table(reads, k, canonical), canonical, *rng)
    assert (u.seqs, u.abund, u.flags, u.summary) == (seqs, abund, flags, words)
    assert u.bases == "".join(seqs) and u.offsets == [0] + list(np.cumsum([len(s) for s in seqs]))


def _random_reads(rng, k):
    """the reads of test_graph_host, and circular ones"""
    rnd = lambda n: "".join("ACGT"[i] for i in rng.integers(0, 4, n))
    reads = [rnd(int(rng.integers(k, k + 40))) for _ in range(12)]
    reads.append(reads[0][: k + 10] + rnd(15))                                   # a fork off the first read
    reads.append(gm.revcomp(reads[1][3: k + 20]))
    reads.append("A" * (k + 4))
    reads.append(("AT" * (k + 4))[: k + 7])
    reads.append(reads[2])                                                       # counts above 1
    if k % 2 == 0:
        half = rnd(k // 2)
        reads.append("G" + half + gm.revcomp(half) + "C")                        # a palindromic k-mer inside
    for n in (k + 9, 2):
        s = rnd(n)
        reads += [(s * (k + 2))[:n + k + 2]] * 2
    return reads


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 7, 8, 21])
def test_model_properties_on_random_reads(k):
    rng = np.random.default_rng(2000 + k)
    for canonical in (True, False):
        for trial in range(3):
            table = gm.count_table(_random_reads(rng, k), k, canonical)
            row = {x: i for i, x in enumerate(sorted(table))}
            for lo, hi in ((1, 0), (2, 0), (1, 1), (2, 3)):
                u = um.unitigs(table, canonical, lo, hi)
                solid = gm.solid_set(table, lo, hi)
                g = gm.graph(table, canonical, lo, hi)[2]
                w = u.summary
                # the k-mers of the unitigs are exactly the solid keys, each once
                km = um.kmers_of(u, k, canonical)
                assert len(km) == len(solid) and set(km) == solid
                # the identities of the contract
                assert w[0] == len(u.seqs) and w[2] == len(solid) == g[0]
                assert w[1] == w[2] + (k - 1) * w[0]
                assert 2 * w[0] == g[6] + w[6] + 2 * w[3]
                assert w[7] == sum(table[x] for x in solid) == sum(u.abund)
                assert w[4] == sum(1 for s in u.seqs if len(s) == k) and w[5] == max([len(s) - k + 1 for s in u.seqs], default=0)
                if not canonical:
                    assert w[6] == 0 and all(s[:k] in solid for s in u.seqs)
                # unitigs ascend by the row of their first key
                first = [row[gm.canon(s[:k], canonical)] for s in u.seqs]
                assert first == sorted(first) and len(set(first)) == len(first)
                # a circular unitig closes on itself, and starts at its smallest row
                for s, f in zip(u.seqs, u.flags):
                    rows = [row[gm.canon(s[j:j + k], canonical)] for j in range(len(s) - k + 1)]
                    if f:
                        assert s[len(s) - k + 1:] + s[k - 1] == s[:k]      # the k-mer after the last one is the first
                        assert rows[0] == min(rows)
                    elif canonical:
                        assert rows[0] <= rows[-1]
