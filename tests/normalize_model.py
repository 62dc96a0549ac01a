"""kmc_normalize restated on Python strings (include/kmc.h): the count of every window of a read against a table, the read's
depth as a percentile of the counts of its valid windows, the unit's depth, the draw, LOW / DEEP / KEEP / EMITTED, the emitted
batch and the summary.  Written from the header; nothing here shares code with the kernels.  CPU only."""
import graph_model as gm

PAIRED, INVERT = 1, 2
KEEP, EMITTED, LOW, DEEP = 1, 2, 4, 8
SAT = 0xFFFFFFFF
M64 = (1 << 64) - 1
_ACGT = frozenset("ACGT")


def window_counts(read, k, canonical, table):
    """per window of the read: None if it is not valid, else the table's count of its key, 0 if absent, saturated"""
    out = []
    for j in range(len(read) - k + 1):
        f = read[j:j + k]
        out.append(min(table.get(gm.canon(f, canonical), 0), SAT) if _ACGT.issuperset(f) else None)
    return out


def depth(counts, permille):
    """(V, d_r) of a read's window counts"""
    c = sorted(x for x in counts if x is not None)
    if not c:
        return 0, 0
    return len(c), c[((len(c) - 1) * permille) // 1000]


def draw(seed, g, D):
    x = (seed + (g + 1) * 0x9E3779B97F4A7C15) & M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return ((x >> 32) * D) >> 32


def judge(D, u, target, min_depth):
    """(keep, low, deep) of a unit"""
    low = D < min_depth
    deep = (not low) and target != 0 and D > target
    return (not low) and ((not deep) or u < target), low, deep


class Normalized:
    """out (strings), origin, stats [n_reads][4], verdict [n_reads], summary [8], offsets [n_out + 1]"""

    def __init__(self, reads, counts, permille=500, target=0, min_depth=0, seed=0, flags=0):
        assert 0 <= permille <= 1000 and not flags & ~3 and not (flags & PAIRED and len(reads) & 1)
        self.reads = list(reads)
        vd = [depth(c, permille) for c in counts]
        self.stats, self.verdict = [], []
        for r in range(len(self.reads)):
            V, d = vd[r]
            D, g = (min(d, vd[r ^ 1][1]), r >> 1) if flags & PAIRED else (d, r)
            u = draw(seed, g, D)
            keep, low, deep = judge(D, u, target, min_depth)
            em = keep != bool(flags & INVERT)
            self.stats.append([V, d, D, u])
            self.verdict.append((KEEP if keep else 0) | (EMITTED if em else 0) | (LOW if low else 0) | (DEEP if deep else 0))
        self.origin = [r for r, v in enumerate(self.verdict) if v & EMITTED]
        self.out = [self.reads[r] for r in self.origin]
        self.offsets = [0]
        for s in self.out:
            self.offsets.append(self.offsets[-1] + len(s))
        n = lambda bits: sum(1 for v in self.verdict if v & bits == bits)
        self.summary = [len(self.reads), sum(s[0] for s in self.stats), len(self.out), self.offsets[-1], n(LOW), n(DEEP), n(DEEP | KEEP),
                        sum(s[1] for s in self.stats)]

    def text(self):
        """what ``k-mer-count --normalize`` prints"""
        return "".join(">%d %d %d %d\n%s\n" % (r, *self.stats[r][:3], s) for r, s in zip(self.origin, self.out))


def all_counts(table, canonical, reads, k):
    return [window_counts(r, k, canonical, table) for r in reads]


def normalize_reads(table, canonical, reads, k=None, counts=None, **rule):
    """table: {k-mer string: count}; k is needed for an empty table; counts: those of an earlier call on the same table and
    reads; rule: permille, target, min_depth, seed, flags"""
    if k is None:
        k = len(next(iter(table)))
    return Normalized(reads, counts if counts is not None else all_counts(table, canonical, reads, k), **rule)
