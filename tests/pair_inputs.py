"""Inputs of the pairs tests (tests/test_pairs_host.py, tests/test_pairs_gpu.py): each gives (the reads that are counted,
the pairs laid on their graph) -- the pairs as a list of Pair records whose .a / .b are the two mates and whose other fields
say how they were cut.  reads_of() flattens them to the interleaved batch the library takes.  CPU only; nothing here touches
the library."""
from collections import namedtuple

import numpy as np

import graph_model as gm
from map_inputs import rnd

# kind: "fr" a forward / reverse pair off one fragment, "junk", "same", "everted", "tie", "ff"; frag: the fragment length a
# pair was cut with (0 where that means nothing)
Pair = namedtuple("Pair", "a b kind frag")


def reads_of(pairs):
    out = []
    for p in pairs:
        out += [p.a, p.b]
    return out


def mate_len(rng, k):
    return int(rng.integers(max(40, k + 5), max(100, k + 40) + 1))


def cut(rng, g, k, lo, hi, fmin=150, fmax=400):
    """a forward / reverse pair off a fragment of g[lo:hi] on a random strand"""
    F = int(rng.integers(fmin, fmax + 1))
    p = int(rng.integers(lo, hi - F + 1))
    frag = g[p:p + F]
    if rng.integers(0, 2):
        frag = gm.revcomp(frag)
    return Pair(frag[:mate_len(rng, k)], gm.revcomp(frag)[:mate_len(rng, k)], "fr", F)


def variant(rng, s):
    p = len(s) // 2
    return s[:p] + "ACGT"[("ACGT".index(s[p]) + 1 + int(rng.integers(0, 3))) % 4] + s[p + 1:]


# the genome of library / edges: substitutions are counted in its first BUSY bases only, the rest is one long unitig
GENOME, BUSY = 1500, 800


def _sample(rng, k):
    g = rnd(rng, GENOME)
    w = 2 * k + 20
    sample = [g]
    for p in range(30, BUSY - w, max(60, w // 2)):        # a counted substitution every 60 bases or so: many unitigs
        sample.append(variant(rng, g[p:p + w]))
    return g, sample


def specials(rng, g, k):
    """the pairs that are no ordinary forward / reverse pair, all cut from the long unitig behind g[BUSY + k:]: junk (UNPLACED),
    same (SAME_STRAND), everted (EVERTED), tie (mate A has two equally long segments and is anchored on the second)"""
    lo = BUSY + k + 5
    frag = g[lo + 20:lo + 20 + 300]
    la, lb = mate_len(rng, k), mate_len(rng, k)
    n = 12
    t = g[lo + 30:lo + 30 + 2 * (k - 1 + n) + 1]
    t = t[:k - 1 + n] + "N" + t[k + n:]
    return [Pair(rnd(rng, la), gm.revcomp(frag)[:lb], "junk", 0),
            Pair(frag[:la], frag[-lb:], "same", 0),
            Pair(frag[-la:], gm.revcomp(frag[:lb]), "everted", 0),
            Pair(t, gm.revcomp(g[lo + 30:lo + 430])[:lb], "tie", 400)]


def library(k, seed, n_pairs=200):
    rng = np.random.default_rng(seed)
    g, sample = _sample(rng, k)
    pairs = [cut(rng, g, k, 0, GENOME) for _ in range(n_pairs)]
    for _ in range(20):                                   # both mates on the forward strand: SPAN in a forward ctx too
        p = cut(rng, g, k, 0, GENOME)
        pairs.append(Pair(p.a, gm.revcomp(p.b), "ff", 0))
    return sample, pairs + specials(rng, g, k)


def gap(k, seed, g, n_pairs=100, side=600):
    """two stretches P, Q counted separately, fragments across an uncounted gap of g bases between them"""
    rng = np.random.default_rng(seed)
    G = rnd(rng, 2 * side + g)
    P, Q = G[:side], G[side + g:]
    pairs = []
    for _ in range(n_pairs):
        F = int(rng.integers(g + 2 * (k + 45), g + 2 * (k + 45) + 200))
        p = int(rng.integers(max(0, side + g + k + 41 - F), side - (k + 41) + 1))     # mate A inside P, mate B inside Q
        frag = G[p:p + F]
        la, lb = min(mate_len(rng, k), side - p), min(mate_len(rng, k), p + F - side - g)
        a, b = frag[:la], gm.revcomp(frag)[:lb]
        pairs.append(Pair(b, a, "fr", F) if rng.integers(0, 2) else Pair(a, b, "fr", F))
    return [P, Q], pairs


def adjacent(k, seed, n_pairs=100, side=600):
    """A + B counted with a second way out of A, so A and B are two unitigs joined by a link; error-free pairs across it,
    every mate on one side of it"""
    rng = np.random.default_rng(seed)
    A, B, C = rnd(rng, side), rnd(rng, side), rnd(rng, k + 30)
    G = A + B
    pairs = []
    for _ in range(n_pairs):
        la, lb = mate_len(rng, k), mate_len(rng, k)
        p = int(rng.integers(side - la - 150, side - la + 1))
        e = int(rng.integers(side + lb + k, side + lb + k + 150))
        frag = G[p:e]
        a, b = frag[:la], gm.revcomp(frag)[:lb]
        pairs.append(Pair(b, a, "fr", e - p) if rng.integers(0, 2) else Pair(a, b, "fr", e - p))
    return [G, A[-(k + 10):] + C], pairs


def hot(k, seed, n):
    """n pairs that all land on one record"""
    return gap(k, seed, 50, n_pairs=n)


_TWO = {}


def two_unitigs(k, seed):
    """(S, T): two strings that are exactly two unitigs, of 3k + 5 and 2k + 2 keys, when counted canonically and when counted
    forward -- at k = 5 and 6 a random kilobase is a tangle, so the small graph is searched for, seed by seed, with the model"""
    import unitig_model as um
    if (k, seed) not in _TWO:
        for s in range(seed, seed + 100000):
            rng = np.random.default_rng(s)
            S, T = rnd(rng, 4 * k + 4), rnd(rng, 3 * k + 1)
            if all(sorted(len(x) for x in um.unitigs(gm.count_table([S, T], k, c), c).seqs) == [len(T), len(S)] for c in (True, False)):
                _TWO[(k, seed)] = (S, T)
                break
    return _TWO[(k, seed)]


def small_specials(k, S, T):
    """on the two unitigs S and T, mates of 2k bases: junk (UNPLACED: a mate of N), same (SAME_STRAND: one mate twice), self
    (PROPER: a mate and its own reverse complement, F the mate length), everted (EVERTED), tie (PROPER across all of S, mate A
    in two equally long segments), span (SPAN) and ff (SPAN in a forward ctx too: both mates forward)"""
    n = 2 * k
    t = S[:2 * (k + 1) + 1]
    t = t[:k + 1] + "N" + t[k + 2:]
    return [Pair("N" * (k + 3), gm.revcomp(S)[:n], "junk", 0),
            Pair(S[:n], S[:n], "same", 0),
            Pair(S[2:2 + n], gm.revcomp(S[2:2 + n]), "self", n),
            Pair(S[-n:], gm.revcomp(S[:n]), "everted", 0),
            Pair(t, gm.revcomp(S)[:n], "tie", len(S)),
            Pair(S[:n], gm.revcomp(T)[:n], "span", 0),
            Pair(S[:n], T[:n], "ff", 0)]


def small(k, seed, n_pairs=40):
    """every class on a graph of two unitigs, at every k: forward / reverse pairs off fragments of S, then small_specials"""
    S, T = two_unitigs(k, seed)
    rng = np.random.default_rng(seed)
    pairs = []
    for _ in range(n_pairs):
        F = int(rng.integers(2 * k, len(S) + 1))
        p = int(rng.integers(0, len(S) - F + 1))
        frag = S[p:p + F] if rng.integers(0, 2) else gm.revcomp(S[p:p + F])
        pairs.append(Pair(frag[:2 * k], gm.revcomp(frag)[:2 * k], "fr", F))
    return [S, T], pairs + small_specials(k, S, T)


EDGE_AT = (63, 64, 65, 255, 256, 257)
EDGE_CLASS = {"junk": 0, "same": 4, "self": 2, "everted": 3, "tie": 2}      # what a special pair at a seam is, canonical


def edges(k, seed):
    """the special pairs at the wave and workgroup seams of a batch of 300 ordinary ones (k < 31: on the two small unitigs)"""
    if k < 31:
        sample, pairs = small(k, seed, n_pairs=300)
        pairs, sp = pairs[:300], pairs[300:]
        for j, at in enumerate(EDGE_AT):
            pairs[at] = sp[j % 5]
        return sample, pairs
    rng = np.random.default_rng(seed)
    g, sample = _sample(rng, k)
    pairs = [cut(rng, g, k, 0, GENOME) for _ in range(300)]
    sp = specials(rng, g, k)
    for j, at in enumerate(EDGE_AT):
        pairs[at] = sp[j % len(sp)]
    return sample, pairs


def many_records(k, seed, genome=40000, n_pairs=6000):
    """a longer genome with a counted substitution every 60 bases or so: more distinct records than one sort leaf holds"""
    rng = np.random.default_rng(seed)
    g = rnd(rng, genome)
    w = 2 * k + 20
    sample = [g] + [variant(rng, g[p:p + w]) for p in range(30, genome - w, 60)]
    return sample, [cut(rng, g, k, 0, genome) for _ in range(n_pairs)]
