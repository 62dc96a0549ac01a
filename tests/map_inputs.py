"""Inputs of the map tests (tests/test_map_host.py, tests/test_map_gpu.py): each gives (the reads that are counted, the reads
that are laid on their graph) as lists of strings.  CPU only; nothing here touches the library."""
import numpy as np

import graph_model as gm


def rnd(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def genome_reads(k, seed, n_reads=200, genome=3000):
    """Random reads of 40-200 bases off a random genome, each on a random strand; the same reads are mapped back, so both
    orientations and decreasing positions occur.  Behind them the reads that leave gaps: an N, lower-case bytes, reads
    shorter than k, of exactly k bases and empty, and reads of a second sample with one substitution each.  Ten substituted reads are
    counted as well, so that the graph has bubbles and the reads cross from one unitig into the next."""
    rng = np.random.default_rng(seed)
    g = rnd(rng, genome)
    sample = []
    for _ in range(n_reads):
        n = int(rng.integers(max(40, k), 201))
        p = int(rng.integers(0, genome - n + 1))
        s = g[p:p + n]
        sample.append(gm.revcomp(s) if rng.integers(0, 2) else s)
    def variant(s):
        p = int(rng.integers(0, len(s)))
        return s[:p] + "ACGT"[("ACGT".index(s[p]) + 1 + int(rng.integers(0, 3))) % 4] + s[p + 1:]
    sample += [variant(s) for s in sample[:10]]     # counted too: the graph branches, so reads cross from unitig to unitig
    other = [variant(s) for s in sample[10:40]]     # a second sample: k unplaced windows each, or a second arm
    a, b = sample[0], sample[1]
    gaps = [a[:len(a) // 2] + "N" + a[len(a) // 2 + 1:], b[:20] + b[20:24].lower() + b[24:], a[:k - 1], a[:k], "", a[:1] if k > 1 else "",
            "N" * (k + 3), ""]
    return sample, sample + gaps + other


def one_long_unitig(k, seed, length=3100, read=3000):
    """One read along one unitig of more than two chunks of keys, and the same read on the other strand"""
    g = rnd(np.random.default_rng(seed), length)
    return [g], [g[:read], gm.revcomp(g[:read]), g[50:50 + read]]


def two_graphs(k, seed, n_reads=100, stretch=40, stretches=10):
    """Reads that alternate between stretches of a genome that is counted and of one that is not: every stretch on the first
    is a segment of its own, hundreds of them on either side of every compaction tile's edge"""
    rng = np.random.default_rng(seed)
    a, b = rnd(rng, 4000), rnd(rng, 4000)
    reads = []
    for _ in range(n_reads):
        parts = []
        for i in range(stretches):
            src = a if i % 2 == 0 else b
            n = stretch + k - 1 + int(rng.integers(0, 7))
            p = int(rng.integers(0, len(src) - n))
            parts.append(src[p:p + n])
        reads.append("".join(parts))
    return [a], reads


def circular(k, seed, m=50):
    """A cycle of m keys read twice round (the break lies at the cut, with a crossing there), and a homopolymer over a
    one-key circular unitig on both strands (every window is a segment of its own)"""
    c = rnd(np.random.default_rng(seed), m)
    sample = [(c * (k + 2))[:m + k + 2]] * 2 + ["A" * (k + 20)]
    whole = c * (k + 4)
    reads = [whole[:2 * m + k - 1], gm.revcomp(whole[3:2 * m + k + 9]), "A" * (k + 10), "T" * (k + 10), whole[m // 2:m // 2 + k + 5]]
    return sample, reads


def hairpin(k, seed, arm=60):
    """Canonical, odd k: a read that runs into a key whose extension is its own reverse complement and comes back along
    the same unitig on the other strand"""
    assert k % 2 == 1
    w = rnd(np.random.default_rng(seed), arm)
    r = w + gm.revcomp(w)
    return [r], [r, r[10:-3], gm.revcomp(r)[5:]]


def pack(reads):
    bases = np.frombuffer("".join(reads).encode(), np.uint8)
    offs = np.zeros(len(reads) + 1, np.uint64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return bases, offs
