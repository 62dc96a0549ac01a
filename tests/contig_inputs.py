"""Inputs of the contig tests (tests/test_contigs_host.py, tests/test_contigs_gpu.py): each gives a Case -- the reads that are
counted, the reads that are walked through their graph, and what is known about the answer: the linear or circular genomes
the contigs must spell (up to strand), or nothing.  CPU only; nothing here touches the library."""
from collections import namedtuple

import numpy as np

import graph_model as gm
import map_inputs as mi
import transit_inputs as ti
from map_inputs import rnd

Case = namedtuple("Case", "sample reads genomes circular")   # genomes: None where the answer is not a list of genomes
LONG_KS = (31, 32, 33, 63)
W = 20          # flank bases of a spanning read on either side of a repeat
SPREAD = 5      # spanning reads at offsets -SPREAD..SPREAD


def _other(base):
    return "ACGT"[("ACGT".index(base) + 1) % 4]


def _part(x, y):
    """y changed so that it differs from x in its first and in its last base: two genomes part exactly at a repeat's edge"""
    y = (_other(x[0]) + y[1:])
    return y[:-1] + _other(x[-1])


def _tiled(g, n, step):
    """reads of n bases off g at every step-th position, and the last n bases, each on both strands"""
    starts = list(range(0, len(g) - n + 1, step))
    if starts[-1] != len(g) - n:
        starts.append(len(g) - n)
    return [x for p in starts for x in (g[p:p + n], gm.revcomp(g[p:p + n]))]


def _spanning(g, at, n_repeat, w=W, spread=SPREAD):
    """reads that span g[at : at + n_repeat] with about w bases of either flank, each on both strands"""
    out = []
    for off in range(-spread, spread + 1):
        s = g[at - w + off:at + n_repeat + w + off]
        assert len(s) == n_repeat + 2 * w
        out += [s, gm.revcomp(s)]
    return out


def repeat(k, seed):
    sample, reads = ti.repeat(k, seed)
    return Case(sample, reads, sample, False)


def short(k, seed):
    return Case(*ti.short(k, seed), None, False)


def chimera(k, seed):
    return Case(*ti.chimera(k, seed), None, False)


def tandem(k, seed, copies=2):
    """A R R B: the repeat's unitig is entered from A and from the keys across the R|R seam, and left through those keys and
    into B; reads of |R| + 2k bases tiled at step 3 pair every way in with its way out"""
    rng = np.random.default_rng(seed)
    a, b, r = rnd(rng, 80), rnd(rng, 80), rnd(rng, k + 12)
    g = a + r * copies + b
    return Case([g], _tiled(g, len(r) + 2 * k, 3), [g] if copies == 2 else None, False)


def tandem3(k, seed):
    """A R R R B: the way in from the seam goes with two ways out -- AMBIGUOUS, nothing is duplicated"""
    return tandem(k, seed, 3)


def plasmids(k, seed):
    """Two circular genomes R A and R C that share R, counted as g + g[:k-1], walked by reads tiled across the wrap"""
    rng = np.random.default_rng(seed)
    r, a, c = rnd(rng, k + 12), rnd(rng, 90), rnd(rng, 75)
    c = _part(a, c)
    genomes = [r + a, r + c]
    n = len(r) + 2 * k
    reads = [x for g in genomes for x in _tiled(g + g[:n], n, 3)]
    return Case([g + g[:k - 1] for g in genomes], reads, genomes, True)


def two_repeats(k, seed):
    """A R1 M R2 B and C R1 E R2 D"""
    rng = np.random.default_rng(seed)
    a, m, b, c, e, d = (rnd(rng, 80) for _ in range(6))
    r1, r2 = rnd(rng, k + 12), rnd(rng, k + 7)
    c, e, d = c[:-1] + _other(a[-1]), _part(m, e), _other(b[0]) + d[1:]
    genomes = [a + r1 + m + r2 + b, c + r1 + e + r2 + d]
    return Case(genomes, [x for g in genomes for x in _tiled(g, len(r1) + 2 * k, 3)], genomes, False)


def hairpin(k, seed):
    """A + revcomp(A), odd k: canonical, the unitig folds back onto itself at a record that is no join"""
    sample, reads = mi.hairpin(k, seed)
    return Case(sample, reads, None, False)


def ladder(k, seed, gadgets=32):
    """`gadgets` independent two-genome gadgets in one sample: flanks of 60 + i bases and |R| = k + 1 + (i mod 16), so the
    shared unitig has 2..17 keys and every unitig starts at another residue mod 16 in both arrays; one more gadget with
    |R| = k, whose shared unitig is a single key"""
    rng = np.random.default_rng(seed)
    genomes, reads = [], []
    for i in range(gadgets + 1):
        n = 60 + i
        a, b, c, d = (rnd(rng, n) for _ in range(4))
        c, d = c[:-1] + _other(a[-1]), _other(b[0]) + d[1:]
        r = rnd(rng, k + 1 + i % 16 if i < gadgets else k)
        for g in (a + r + b, c + r + d):
            genomes.append(g)
            reads += _spanning(g, n, len(r), spread=2)
    return Case(genomes, reads, genomes, False)


def chain(k, seed, repeats=130, circular=False):
    """Two genomes that share `repeats` repeats in series: F0 R0 F1 R1 ... and G0 R0 G1 R1 ...; every contig is a path (or, in
    the circular form, a cycle) of 2 * repeats + 1 (2 * repeats) nodes.  Flanks of 40 bases, |R| = k + 2 (three keys), two
    spanning reads per strand, repeat and genome."""
    rng = np.random.default_rng(seed)
    rs = [rnd(rng, k + 2) for _ in range(repeats)]
    n_flanks = repeats if circular else repeats + 1
    f = [rnd(rng, 40) for _ in range(n_flanks)]
    g = [_part(x, rnd(rng, 40)) for x in f]
    genomes = []
    for flanks in (f, g):
        s = "".join(flanks[i] + rs[i] for i in range(repeats)) + ("" if circular else flanks[repeats])
        genomes.append(s)
    reads = []
    for s in genomes:
        ext = s + s[:200] if circular else s
        for i in range(repeats):
            at = 40 * (i + 1) + (k + 2) * i
            reads += _spanning(ext, at, k + 2, w=10, spread=1)[:4]
    sample = [s + s[:k - 1] for s in genomes] if circular else genomes
    return Case(sample, reads, genomes, circular)


def chain_circular(k, seed):
    return chain(k, seed, circular=True)


def tangle(k, seed):
    """Random genomes at a k where the graph is dense: repeats with up to 4 x 4 matrices, missing records, palindromes"""
    rng = np.random.default_rng(seed)
    genomes = [rnd(rng, 160), rnd(rng, 120)]
    reads = []
    for _ in range(60):
        g = genomes[int(rng.integers(0, 2))]
        n = int(rng.integers(k + 2, 50))
        p = int(rng.integers(0, len(g) - n + 1))
        reads.append(gm.revcomp(g[p:p + n]) if rng.integers(0, 2) else g[p:p + n])
    return Case(genomes, reads, None, False)


# name -> (the function, the k it is defined at)
INPUTS = {
    "repeat": (repeat, (5, 6) + LONG_KS), "short": (short, (5, 6) + LONG_KS), "chimera": (chimera, (5, 6) + LONG_KS),
    "tandem": (tandem, LONG_KS), "tandem3": (tandem3, LONG_KS), "plasmids": (plasmids, LONG_KS), "two_repeats": (two_repeats, LONG_KS),
    "hairpin": (hairpin, (31, 33, 63)), "ladder": (ladder, LONG_KS), "chain": (chain, (31,)), "chain_circular": (chain_circular, (31,)),
    "tangle": (tangle, (5, 6)),
}
SPELL_GENOMES = ("repeat", "tandem", "two_repeats", "ladder", "chain")     # at k >= 31: the contigs are the genomes, up to strand
NOTHING_DUPLICATED = ("tandem3", "short", "chimera")


def cases(ks=None):
    """(name, k) of every input at every k it is defined at"""
    return [(name, k) for name, (_, at) in INPUTS.items() for k in at if ks is None or k in ks]


def make(name, k):
    return INPUTS[name][0](k, 500 + k)
