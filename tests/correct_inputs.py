"""Inputs of the correction tests (tests/test_correct_host.py, tests/test_correct_gpu.py): each gives (the reads that are
counted, the reads that are corrected) as lists of strings.  CPU only; nothing here touches the library."""
import numpy as np

import graph_model as gm
from map_inputs import pack, rnd  # noqa: F401  (pack is part of this module's interface)


def other_base(rng, c):
    return "ACGT"[("ACGT".index(c) + 1 + int(rng.integers(0, 3))) % 4]


def sub(s, p, c=None):
    """s with position p replaced by c (default: the next base)"""
    return s[:p] + (c or "ACGT"[("ACGT".index(s[p]) + 1) % 4]) + s[p + 1:]


def recovery(k, seed, n_reads, read_len, genome=3000):
    """(reads, originals, [error position or None]): reads of one length off a random genome on random strands, one
    substitution in every third read.  The reads themselves are what is counted."""
    rng = np.random.default_rng(seed)
    g = rnd(rng, genome)
    reads, orig, where = [], [], []
    for i in range(n_reads):
        p = int(rng.integers(0, genome - read_len + 1))
        s = g[p:p + read_len]
        if rng.integers(0, 2):
            s = gm.revcomp(s)
        orig.append(s)
        if i % 3 == 0:
            q = int(rng.integers(0, read_len))
            reads.append(sub(s, q, other_base(rng, s[q])))
            where.append(q)
        else:
            reads.append(s)
            where.append(None)
    return reads, orig, where


def genome_reads(k, seed, n_reads=200, genome=3000):
    """About 200 reads of 40-200 bases (250 at k = 63) off a random genome, on random strands, with the substituted forms
    of thirty of them counted in; all of them are corrected, and behind them the gap reads: an N beside a weak run, lower
    case, reads of k - 1, k and k + 1 bases, empty reads, a read of N only."""
    rng = np.random.default_rng(seed)
    g = rnd(rng, genome)
    hi = 251 if k == 63 else 201
    sample = []
    for _ in range(n_reads):
        n = int(rng.integers(max(40, k + 2), hi))
        p = int(rng.integers(0, genome - n + 1))
        s = g[p:p + n]
        sample.append(gm.revcomp(s) if rng.integers(0, 2) else s)

    def variant(s):
        p = int(rng.integers(0, len(s)))
        return sub(s, p, other_base(rng, s[p]))
    bad = [variant(s) for s in sample[:30]]
    a, b = sample[0], sample[1]
    m = len(a) // 2
    gaps = [sub(a[:m] + "N" + a[m + 1:], max(m - 3, 0)),             # an error right before an N: INVALID right border
            sub(a[:m] + "N" + a[m + 1:], min(m + 2, len(a) - 1)),    # ... and right behind one
            b[:20] + b[20:24].lower() + b[24:], a[:k - 1], a[:k], a[:k + 1], sub(a[:k + 1], 0), "", "N" * (k + 3), "",
            sub(sub(b, 5), min(len(b) - 1, 5 + k // 2))]            # two errors closer than k
    return sample + bad, sample + bad + gaps + [variant(s) for s in sample[30:60]]


def placed(k, seed, length=None):
    """One genome read, counted twice, and its copies with substitutions at the places kmc.h tells apart.  Returns (sample,
    reads, {name: read index})."""
    L = length or 4 * k + 7
    g = rnd(np.random.default_rng(seed), L)
    names, reads = {}, []

    def add(name, s):
        names[name] = len(reads)
        reads.append(s)
    add("clean", g)
    add("at_0", sub(g, 0))
    add("at_k-1", sub(g, k - 1))
    add("at_k", sub(g, k))
    add("at_L-k-1", sub(g, L - k - 1))
    add("at_L-k", sub(g, L - k))
    add("at_L-1", sub(g, L - 1))
    add("two_k+1_apart", sub(sub(g, k), 2 * k + 1))
    add("two_k_apart", sub(sub(g, k), 2 * k))
    add("two_k-1_apart", sub(sub(g, k), 2 * k - 1))
    add("before_N", sub(g[:2 * k] + "N" + g[2 * k + 1:], k + 1))       # k - 1 before the N
    mid = g[:2 * k - 1]
    add("weak_end_to_end", sub(mid, k - 1))
    return [g, g], reads, names


def snp(k, seed, length=None):
    """A genome and its one-SNP variant, counted three times and twice; a read with a third base at the SNP"""
    L = length or 3 * k + 5
    rng = np.random.default_rng(seed)
    g = rnd(rng, L)
    p = L // 2
    alt = [c for c in "ACGT" if c != g[p]]
    v = sub(g, p, alt[0])
    return [g] * 3 + [v] * 2, [sub(g, p, alt[1]), g, v], p, g[p], alt[0]


def seams(k, seed):
    """One read of 3000 bases with errors whose weak runs straddle batch positions 1024 and 2048 -- chunk edges, and with one
    chunk per wave the edges between two waves' spans -- or begin right on one; behind it a short filler, so that the third
    read starts at 3072"""
    g = rnd(np.random.default_rng(seed), 3000)
    s = g
    for p in (100, 1010, 1024 + k + 40, 2040, 2047 + k, 2900):
        s = sub(s, p)
    filler = g[:1024 * 3 - 3000]
    return [g, g], [s, filler, sub(g[500:500 + 3 * k], 2 * k), sub(g[:2 * k + 3], 0)]


def starts_at_1024(k, seed):
    """A read of 1024 bases with an error near its end, then reads that start exactly at batch position 1024 and behind"""
    g = rnd(np.random.default_rng(seed), 1400)
    return [g, g], [sub(g[:1024], 1024 - k // 2), sub(g[100:100 + 3 * k], 0), sub(g[200:200 + 3 * k], k), sub(g[300:300 + 3 * k], 3 * k - 1)]


def many_short(k, seed, n=3000):
    """n reads of 2k + 1 bases with an error each at a position that moves through the read: candidates of all three kinds
    on both sides of every compaction tile's edge, and several hundred read starts in one chunk"""
    rng = np.random.default_rng(seed)
    g = rnd(rng, 2000)
    L = 2 * k + 1
    reads = []
    for i in range(n):
        p = int(rng.integers(0, len(g) - L + 1))
        reads.append(sub(g[p:p + L], i % L))
    return [g, g], reads
