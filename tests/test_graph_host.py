"""CPU-side checks of the de Bruijn graph feature: the two entry points are exported and reject a NULL ctx, the CLI rejects
bad uses of --graph / --graph-stats before touching a GPU, GraphSummary's arithmetic and text, and the Python model the GPU
tests compare against (tests/graph_model.py): hand-worked answers for tiny inputs and invariants on random reads."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import graph_model as gm
from conftest import ROOT, SAMPLE

NEW = ("kmc_graph", "kmc_graph_device")
EXE = os.path.join(ROOT, "bin", "k-mer-count")


def test_library_exports_the_graph_calls(kmc):
    out = subprocess.run(["nm", "-D", "--defined-only", kmc.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for s in NEW:
        assert f" T {s}\n" in out, s
        assert s in kmc.ABI_SYMBOLS
    L = kmc.lib()
    a = np.zeros(8, np.uint64)
    p = a.ctypes.data
    n = C.c_uint64(7)
    assert L.kmc_graph(None, 1, 0, p, 4, C.byref(n), p) == kmc.ERR_ARG and n.value == 0 and not a.any()
    assert L.kmc_graph(None, 1, 0, None, 0, None, None) == kmc.ERR_ARG
    assert L.kmc_graph_device(None, 1, 0, None, None, None) == kmc.ERR_ARG
    assert kmc.GRAPH_WORDS == 8 and len(gm.FIELDS) == 8
    assert (kmc.GRAPH_END_R, kmc.GRAPH_END_L, kmc.GRAPH_SOLID) == (gm.END_R, gm.END_L, gm.SOLID)


def test_header_declares_the_graph_section():
    hdr = open(os.path.join(ROOT, "include", "kmc.h")).read()
    assert "#define KMC_GRAPH_WORDS 8" in hdr
    for m in ("KMC_GRAPH_RIGHT", "KMC_GRAPH_LEFT", "KMC_GRAPH_END_R", "KMC_GRAPH_END_L", "KMC_GRAPH_SOLID"):
        assert f"#define {m}(adj)" in hdr, m


@pytest.mark.parametrize("argv", [
    ["--graph"], ["--graph-stats"],                                                    # without -k
    ["-k", "5", "--graph", "--graph-stats"],                                           # both together
    ["-k", "5", "--graph", "--histo", "10"], ["-k", "5", "--graph-stats", "--histo", "10"],
    ["-k", "5", "--graph", "--query-kmers", "KMERS"], ["-k", "5", "--graph-stats", "--query-kmers", "KMERS"],
    ["-k", "5", "--graph", "--profile", "SAMPLE"], ["-k", "5", "--graph-stats", "--profile", "SAMPLE"],
    ["-k", "5", "--graph", "--with", "SAMPLE", "--compare"], ["-k", "5", "--graph-stats", "--with", "SAMPLE", "--compare"],
    ["-k", "5", "--graph", "--with", "SAMPLE", "--setop", "union"], ["-k", "5", "--graph-stats", "--with", "SAMPLE", "--setop", "union"],
    ["-k", "5", "--graph", "--with", "SAMPLE"], ["-k", "5", "--graph", "--compare"], ["-k", "5", "--graph-stats", "--setop", "union"],
    ["-k", "5", "--graph", "--expand"], ["-k", "5", "--graph-stats", "--expand"],
    ["-k", "5", "--graph", "--min-count", "3", "--max-count", "2"]])                    # an empty range, as everywhere
def test_cli_rejects_bad_graph_options(kmc, tmp_path, argv):
    kmers = tmp_path / "kmers.txt"
    kmers.write_text("ACGTA\n")
    argv = [SAMPLE if a == "SAMPLE" else str(kmers) if a == "KMERS" else a for a in argv]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")   # no GPU to touch even where there is one
    r = subprocess.run([EXE, SAMPLE] + argv, capture_output=True, text=True, env=env)
    assert r.returncode == 2 and r.stdout == "" and "k-mer-count:" in r.stderr, (argv, r.returncode, r.stderr)
    assert "unknown option" not in r.stderr, r.stderr      # rejected as a known option in a bad combination


def test_cli_help_lists_graph_options(kmc):
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == ""
    assert "--graph | --graph-stats" in r.stderr


def test_graph_summary_arithmetic_and_text(kmc):
    w = [3260, 3346, 3354, 0, 0, 140, 460, 70]
    s = kmc.GraphSummary.from_words(np.array(w, np.uint64))
    assert s.words() == w and all(type(x) is int for x in s.words())
    assert (s.nodes, s.right_degrees, s.left_degrees, s.isolated, s.dead_ends, s.branching, s.end_sides, s.single_node_unitigs) == tuple(w)
    assert s.unitigs == 230
    assert kmc.GraphSummary.from_words([1, 0, 0, 1, 0, 0, 3, 1]).unitigs == 1    # (odd only for hand-made words: floor)
    text = s.to_text()
    assert text == ("nodes\t3260\nright_degrees\t3346\nleft_degrees\t3354\nisolated\t0\ndead_ends\t0\nbranching\t140\n"
                    "end_sides\t460\nsingle_node_unitigs\t70\nunitigs\t230\n")
    assert text == gm.stats_text(w)
    assert kmc.GraphSummary.from_words([0] * 8).to_text().endswith("unitigs\t0\n")


S, ER, EL = gm.SOLID, gm.END_R, gm.END_L
A, Cc, G, T = 1, 2, 4, 8          # right-extension bits; the left ones are these << 4


@pytest.mark.parametrize("reads,k,canonical,rng,keys,adj,words", [
    # ACG -> CGT -> GTT, one path: its two outer sides are dead ends and the only unitig ends
    (["ACGTT"], 3, False, (1, 0), ["ACG", "CGT", "GTT"], [S | T | EL, S | T | (A << 4), S | (Cc << 4) | ER], [3, 2, 2, 0, 2, 0, 2, 0]),
    # one node whose extension by A on either side is itself: both sides continue (into the node), no end, a circular unitig
    (["AAAAA"], 3, False, (1, 0), ["AAA"], [S | A | (A << 4)], [1, 1, 1, 0, 0, 0, 0, 0]),
    (["AAAAA"], 3, True, (1, 0), ["AAA"], [S | A | (A << 4)], [1, 1, 1, 0, 0, 0, 0, 0]),
    # a fork: AAC -> ACG and AAC -> ACT.  AAC branches (R degree 2), so its R side ends and so do the L sides of both
    # successors (their one neighbour's facing side has degree 2); every node is a unitig of its own
    (["AACG", "AACT"], 3, False, (1, 0), ["AAC", "ACG", "ACT"],
     [S | G | T | ER | EL, S | (A << 4) | ER | EL, S | (A << 4) | ER | EL], [3, 2, 2, 0, 3, 1, 6, 3]),
    # the same with min_count 2: only AAC (seen twice) is solid and it is isolated; the others get 0
    (["AACG", "AACT"], 3, False, (2, 0), ["AAC", "ACG", "ACT"], [S | ER | EL, 0, 0], [1, 0, 0, 1, 0, 0, 2, 1]),
    # ... and with max_count 1: the two successors alone, both isolated
    (["AACG", "AACT"], 3, False, (1, 1), ["AAC", "ACG", "ACT"], [0, S | ER | EL, S | ER | EL], [2, 0, 0, 2, 0, 0, 4, 2]),
    # canonical: CAAG holds CAA (< TTG) and AAG (< CTT).  CAA + G = AAG is kept, so AAG is entered on its L side
    (["CAAG"], 3, True, (1, 0), ["AAG", "CAA"], [S | (Cc << 4) | ER, S | G | EL], [2, 1, 1, 0, 2, 0, 2, 0]),
    # canonical: TTGA holds TTG -> CAA and TGA -> TCA; T + CA(A) = TCA extends CAA to the left
    (["TTGA"], 3, True, (1, 0), ["CAA", "TCA"], [S | (T << 4) | ER, S | A | EL], [2, 1, 1, 0, 2, 0, 2, 0]),
    # a window with an N is not a k-mer: AC and GT do not touch
    (["ACNGT"], 2, False, (1, 0), ["AC", "GT"], [S | ER | EL, S | ER | EL], [2, 0, 0, 2, 0, 0, 4, 2]),
    # k = 1: the overlap is empty, an extension by c is the 1-mer c whatever x is: A and C both have both as neighbours on both sides
    (["AC"], 1, False, (1, 0), ["A", "C"], [S | A | Cc | (A << 4) | (Cc << 4) | ER | EL] * 2, [2, 4, 4, 0, 0, 2, 4, 2]),
])
def test_model_against_hand_written_answers(reads, k, canonical, rng, keys, adj, words):
    table = gm.count_table(reads, k, canonical)
    got = gm.graph(table, canonical, *rng)
    assert got == (keys, adj, words)
    assert gm.graph(table, canonical, *rng, cont=gm.sibling_continues) == got


def test_model_text_forms():
    table = gm.count_table(["AACG", "AACT"], 3, False)
    assert gm.graph_text(table, False) == "AAC\t2\tGT\t.\tLR\nACG\t1\t.\tA\tLR\nACT\t1\t.\tA\tLR\n"
    assert gm.graph_text(table, False, 2, 0) == "AAC\t2\t.\t.\tLR\n"
    assert gm.graph_text(gm.count_table(["ACGTT"], 3, False), False) == "ACG\t1\tT\t.\tL\nCGT\t1\tT\tA\t.\nGTT\t1\t.\tC\tR\n"


def _random_reads(rng, k):
    reads = []
    for _ in range(12):
        n = int(rng.integers(k, k + 40))
        reads.append("".join("ACGT"[i] for i in rng.integers(0, 4, n)))
    reads.append(reads[0][: k + 10] + "".join("ACGT"[i] for i in rng.integers(0, 4, 15)))   # a fork off the first read
    reads.append(gm.revcomp(reads[1][3: k + 20]))
    reads.append("A" * (k + 4))
    reads.append(("AT" * (k + 4))[: k + 7])
    reads.append(reads[2])                                                                  # counts above 1
    if k % 2 == 0:
        half = "".join("ACGT"[i] for i in rng.integers(0, 4, k // 2))
        reads.append("G" + half + gm.revcomp(half) + "C")                                   # a palindromic k-mer inside
    return reads


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 7, 8, 21])
def test_model_invariants_on_random_reads(k):
    rng = np.random.default_rng(1000 + k)
    for canonical in (True, False):
        for trial in range(3):
            table = gm.count_table(_random_reads(rng, k), k, canonical)
            for lo, hi in ((1, 0), (2, 0), (1, 1), (2, 3)):
                keys, adj, w = gm.graph(table, canonical, lo, hi)
                assert keys == sorted(table) and len(adj) == len(keys)
                assert w[0] == len(gm.solid_set(table, lo, hi)) and w[3] + w[4] <= w[0] and w[7] <= w[0] and w[6] <= 2 * w[0]
                if not canonical:
                    assert w[1] == w[2]          # every edge leaves one node to the right and enters one from the left
                # the sibling form (what the kernel computes) is the neighbour form
                assert gm.graph(table, canonical, lo, hi, cont=gm.sibling_continues) == (keys, adj, w)
                # an edge is seen from both of its ends
                solid = gm.solid_set(table, lo, hi)
                for x in solid:
                    for side in "RL":
                        for _, y, facing in gm.neighbours(x, side, canonical, solid):
                            assert any(z == x for _, z, _ in gm.neighbours(y, facing, canonical, solid))
