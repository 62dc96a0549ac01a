"""Inputs of the transit tests (tests/test_transits_host.py, tests/test_transits_gpu.py): each gives (the reads that are
counted, the reads that are walked through their graph) as lists of strings.  CPU only; nothing here touches the library."""
import numpy as np

import graph_model as gm
from map_inputs import rnd

FLANK, SPREAD = 80, 5     # bases on either side of the repeat; read offsets -SPREAD..SPREAD: 11 of them


def _other(base):
    return "ACGT"[("ACGT".index(base) + 1) % 4]


def _genomes(k, seed):
    """A R B and C R D: two genomes that share R, |R| = k + 12, and nothing else"""
    rng = np.random.default_rng(seed)
    a, b, c, d = (rnd(rng, FLANK) for _ in range(4))
    c, d = c[:-1] + _other(a[-1]), _other(b[0]) + d[1:]     # the two genomes part exactly where R begins and ends
    return a, b, c, d, rnd(rng, k + 12)


def _around(g, k, n, centre):
    """reads of n bases off g at the 11 offsets around `centre`, each on both strands"""
    out = []
    for off in range(-SPREAD, SPREAD + 1):
        s = g[centre + off:centre + off + n]
        assert len(s) == n
        out += [s, gm.revcomp(s)]
    return out


def repeat(k, seed):
    """Reads of |R| + 2k bases that span R with about k bases of either flank: every one that lies on the graph's strand is a
    transit of R's unitig, and each way in goes with one way out"""
    a, b, c, d, r = _genomes(k, seed)
    sample = [a + r + b, c + r + d]
    return sample, [x for g in sample for x in _around(g, k, len(r) + 2 * k, FLANK - k)]


def short(k, seed):
    """The same graph under reads of |R| bases: they cross into R or out of it and never do both"""
    a, b, c, d, r = _genomes(k, seed)
    sample = [a + r + b, c + r + d]
    return sample, [x for g in sample for x in _around(g, k, len(r), FLANK)]


def chimera(k, seed):
    """The reads of repeat() and as many of A R D, which is not counted: A goes out through both B and D"""
    a, b, c, d, r = _genomes(k, seed)
    sample, reads = repeat(k, seed)
    return sample, reads + _around(a + r + d, k, len(r) + 2 * k, FLANK - k)


PAIR_DEPTH = 2 * (2 * SPREAD + 1)   # the spanning reads of one (way in, way out) pair of repeat(): 22, half of them per strand


def read_boundary(k, seed, w=20, pairs=200):
    """Pairs of reads (r, r + 1): r is one segment of w windows that ends at its last window; r + 1 begins with w bases that
    are not counted and goes on along another unitig, so its first segment has start == w == the start + len of the segment
    before it -- in another read: no crossing.  Behind one single-segment read the second segment of pair i is segment
    2 + 2i, so the pairs straddle a wave's edge at 64, 128, 192, a workgroup's at 256, and lie inside one wave elsewhere.  The
    last reads cross for real, so the batch has crossings to miscount."""
    rng = np.random.default_rng(seed)
    g1, g2, junk = rnd(rng, 300), rnd(rng, 300), rnd(rng, 300)
    reads = [g1[:w + k - 1]]
    for i in range(pairs):
        p, q = int(rng.integers(0, 300 - (w + k - 1))), int(rng.integers(1, 300 - (k + 10)))
        j = int(rng.integers(0, 300 - w))
        reads += [g1[p:p + w + k - 1], junk[j:j + w - 1] + _other(g2[q - 1]) + g2[q:q + k + 10]]    # (no window before w is one of g2)
    sample, real = repeat(k, seed + 1)
    return [g1, g2] + sample, reads + real
