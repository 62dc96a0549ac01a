"""CPU checks of the map model (tests/map_model.py) that the GPU tests compare kmc_unitig_map against: what it says is held
against the read and unitig strings themselves and against links_model, so a mistake in the model cannot hide behind an equal
mistake in the library.  Also what needs no GPU of the feature's surface: the ABI lists and the CLI's usage error."""
import os
import re
import subprocess

import pytest

import graph_model as gm
import links_model as lm
import map_inputs as mi
import map_model as mm
import unitig_model as um
from conftest import ROOT, SAMPLE

RANGES = ((1, 0), (2, 0), (1, 1), (2, 3))
KS = (5, 6, 31, 32, 33, 63)


def _inputs(k, canonical):
    out = [("genome", mi.genome_reads(k, 100 + k, n_reads=60, genome=1200)), ("circular", mi.circular(k, 200 + k))]
    if k == 31:
        out.append(("two_graphs", mi.two_graphs(k, 300 + k, n_reads=10)))
    if canonical and k % 2 == 1:
        out.append(("hairpin", mi.hairpin(k, 400 + k)))
    return out


def _maps(k, canonical):
    for name, (sample, reads) in _inputs(k, canonical):
        table = gm.count_table(sample, k, canonical)
        for lo, hi in RANGES:
            u = um.unitigs(table, canonical, lo, hi)
            yield name, (lo, hi), table, reads, u, mm.ReadMap(reads, k, canonical, u.seqs)


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", KS)
def test_segments_spell_the_read_and_cover_every_placed_window(k, canonical):
    seen = {"o1": 0, "segments": 0, "crossings": 0, "unplaced_valid": 0}
    for name, rng_, table, reads, u, m in _maps(k, canonical):
        solid = gm.solid_set(table, *rng_)
        for r, read in enumerate(reads):
            segs = m.segments[m.seg_offsets[r]:m.seg_offsets[r + 1]]
            covered, base = [0] * len(read), sum(len(x) for x in reads[:r])
            for start, ln, uni, pos in segs:
                s, o = u.seqs[uni >> 1], uni & 1
                piece = read[start:start + ln + k - 1]
                assert len(piece) == ln + k - 1
                if o == 0:
                    assert piece == s[pos:pos + ln + k - 1], (name, rng_, r, start)
                else:
                    assert pos + k - (ln + k - 1) >= 0 and piece == gm.revcomp(s[pos + k - (ln + k - 1):pos + k]), (name, rng_, r, start)
                for j in range(start, start + ln):
                    covered[j] += 1
                seen["o1"] += o
            # every placed window lies in exactly one segment, and the windows that are not placed in none
            for j in range(len(read)):
                f = read[j:j + k]
                placed = len(f) == k and set(f) <= set("ACGT") and gm.canon(f, canonical) in solid
                assert covered[j] == (1 if placed else 0), (name, rng_, r, j)
                assert (m.place[base + j] & 0xFFFFFFFF != mm.NONE) == placed
            assert m.stats[r][1] == sum(s[1] for s in segs) and m.stats[r][2] == len(segs)
            assert [s[0] for s in segs] == sorted(s[0] for s in segs)
            seen["unplaced_valid"] += m.stats[r][0] - m.stats[r][1]
        # the identities of the summary
        w = m.summary
        assert w[2] == sum(m.support) and w[3] == m.seg_offsets[-1] == len(m.segments) and w[0] == len(reads)
        assert w[1] == sum(s[0] for s in m.stats) and w[4] == sum(s[3] for s in m.stats) and w[1] >= w[2] >= w[3] >= w[4]
        assert len(m.place) == sum(len(x) for x in reads) and len(m.support) == len(u.seqs)
        seen["segments"] += w[3]
        seen["crossings"] += w[4]
    assert seen["segments"] > 0 and seen["crossings"] > 0 and seen["unplaced_valid"] > 0, seen
    assert (seen["o1"] > 0) == canonical, seen


@pytest.mark.parametrize("k,canonical", [(k, c) for k in KS for c in (True, False) if k % 2 == 1 or not c])
def test_crossings_follow_links(k, canonical):
    """a read that steps from one window to the next without a gap and without continuing has walked a link record"""
    n = 0
    for name, rng_, table, reads, u, m in _maps(k, canonical):
        lk = lm.links(table, canonical, *rng_)
        keys = [len(s) - k + 1 for s in u.seqs]
        for r in range(len(reads)):
            segs = m.segments[m.seg_offsets[r]:m.seg_offsets[r + 1]]
            for a, b in zip(segs, segs[1:]):
                if b[0] != a[0] + a[1]:
                    continue   # a gap lies between them
                (u1, o1), (u2, o2) = (a[2] >> 1, a[2] & 1), (b[2] >> 1, b[2] & 1)
                last = a[3] + a[1] - 1 if o1 == 0 else a[3] - (a[1] - 1)
                assert last == (keys[u1] - 1 if o1 == 0 else 0), (name, rng_, r, a, b)        # the last key of u in reading direction
                assert b[3] == (0 if o2 == 0 else keys[u2] - 1), (name, rng_, r, a, b)        # the first key of v in its direction
                e, e2 = 2 * u1 + 1 - o1, 2 * u2 + o2
                assert e2 in lk.to[lk.offsets[e]:lk.offsets[e + 1]], (name, rng_, r, a, b)
                n += 1
    assert n > 0


def test_shapes_are_what_they_claim():
    k = 31
    sample, reads = mi.one_long_unitig(k, 7)
    table = gm.count_table(sample, k, True)
    m = mm.map_reads(table, True, reads)
    assert um.unitigs(table, True).summary[5] > 2100
    assert [s[2] for s in m.stats] == [1, 1, 1] and m.summary[4] == 0 and {s[2] & 1 for s in m.segments} == {0, 1}
    assert all(s[1] == len(r) - k + 1 for s, r in zip(m.segments, reads))
    sample, reads = mi.circular(k, 8)
    table = gm.count_table(sample, k, True)
    u = um.unitigs(table, True)
    m = mm.map_reads(table, True, reads)
    assert sorted(u.flags) == [1, 1] and 1 in [len(s) - k + 1 for s in u.seqs]
    # twice round, 2 m windows: the cut is crossed twice (once if the read starts right behind it), the breaks lie at the cut
    first = m.read_segments[0]
    assert m.stats[0][1] == 100 and m.stats[0][2] in (2, 3) and m.stats[0][3] == m.stats[0][2] - 1
    assert all(a[2] == b[2] and ((a[3] + a[1] == 50 and b[3] == 0) if a[2] & 1 == 0 else (a[3] - a[1] + 1 == 0 and b[3] == 49))
               for a, b in zip(first, first[1:]))
    assert m.stats[2][2] == m.stats[2][0] == 11 and m.stats[2][3] == 10   # the homopolymer: every window on its own
    assert m.stats[3][2] == 11 and all(s[2] & 1 for s in m.read_segments[3])
    sample, reads = mi.hairpin(k, 9)
    m = mm.map_reads(gm.count_table(sample, k, True), True, reads)
    assert m.stats[0][1] == m.stats[0][0] and m.stats[0][2] == 2 and m.stats[0][3] == 1
    assert sorted(s[2] & 1 for s in m.read_segments[0]) == [0, 1] and m.read_segments[0][0][2] >> 1 == m.read_segments[0][1][2] >> 1
    sample, reads = mi.two_graphs(k, 10)
    m = mm.map_reads(gm.count_table(sample, k, False), False, reads)
    assert m.summary[3] >= 500 and m.summary[4] == 0 and len("".join(reads)) > 3 * 2048
    assert m.text().count("\n") == len(reads) and m.walks()[0][0][0][3] >= 40


def test_abi_lists_hold_the_map_calls(kmc):
    names = ("kmc_unitig_map", "kmc_unitig_map_device")
    assert all(n in kmc.ABI_SYMBOLS for n in names)
    with open(os.path.join(ROOT, "rust", "src", "lib.rs")) as f:
        rs = f.read()
    assert all(re.search(r"pub fn %s\(" % n, rs) for n in names) and "pub fn map_reads(" in rs
    with open(os.path.join(ROOT, "include", "kmc.h")) as f:
        hdr = f.read()
    assert "#define KMC_MAP_WORDS %d" % kmc.MAP_WORDS in hdr and "#define KMC_MAP_READ_WORDS %d" % kmc.MAP_READ_WORDS in hdr
    assert hasattr(kmc.KmerCounter, "map_reads") and hasattr(kmc.KmerCounter, "map_reads_device") and hasattr(kmc.ReadMap, "walks")
    assert kmc.MapSummary.from_words(range(8)).words() == list(range(8))


def test_cli_rejects_map_without_k(kmc):
    exe = os.path.join(ROOT, "bin", "k-mer-count")
    for argv in (["--map", "x"], ["--map"], ["-k", "31", "--map", "x", "--gfa"], ["-k", "31", "--map", "x", "--profile", "y"],
                 ["-k", "31", "--map", "x", "--histo", "5"]):
        r = subprocess.run([exe, SAMPLE] + argv, capture_output=True, text=True)
        assert r.returncode == 2 and r.stdout == "" and "k-mer-count:" in r.stderr, (argv, r.returncode, r.stderr)
    r = subprocess.run([exe, SAMPLE, "--map", "x"], capture_output=True, text=True)
    assert "--map needs -k K" in r.stderr
