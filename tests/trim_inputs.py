"""Inputs of the trim tests (tests/test_trim_host.py, tests/test_trim_gpu.py): each gives (the reads that are counted, the
reads that are trimmed) as lists of strings, some with a dict of names.  CPU only; nothing here touches the library."""
import numpy as np

from correct_inputs import genome_reads, many_short, starts_at_1024, sub  # noqa: F401  (part of this module's interface)
from map_inputs import pack, rnd  # noqa: F401

# the reduce kernel's variants (kmc_trim.hip.h: KMC_TR_LANE_MAX, KMC_TR_WAVE_MAX), in windows
LANE_MAX, WAVE_MAX = 1024, 32768


def with_holes(g, k, missing):
    """Pieces of g that hold every window of g but those that start at `missing` (ascending, at least 2 apart, none at 0 or
    at the last window): counted, they leave exactly those windows of g without a count"""
    cuts = [-1] + list(missing) + [len(g) - k + 1]
    return [g[a + 1:b + k - 1] for a, b in zip(cuts, cuts[1:])]


def shapes(k, seed):
    """A genome counted twice but for three windows m1 < m2 < m3, d apart, and reads named by the shape of their strong
    runs.  Returns (sample, reads, {name: read index}, d)."""
    rng = np.random.default_rng(seed)
    d = 2 * k + 8                                     # (a run of d - 1 windows outlasts the k windows an N takes)
    g = rnd(rng, 4 * d + 3 * k)
    m1, m2, m3 = d, 2 * d, 3 * d
    names, reads = {}, []

    def add(name, s):
        names[name] = len(reads)
        reads.append(s)
    whole = g[m1 + 1:m2 + k - 1]                      # windows m1 + 1 .. m2 - 1
    add("all_strong", whole)
    add("none_strong", rnd(rng, len(whole)))
    add("weak_at_0", g[m1:m2 + k - 1])
    add("weak_at_last", g[m1 + 1:m2 + k])
    add("weak_in_the_middle", g[m1 + 1:m3 + k - 1])   # two longest runs of d - 1 windows: the first wins
    add("longest_run_last", g[m2 - 5:m3 + k - 1])     # 5 strong, one weak, d - 1 strong
    q = len(whole) // 2
    add("split_by_N", whole[:q] + "N" + whole[q + 1:])
    add("ends_with_weak_inside", g)
    return with_holes(g, k, (m1, m2, m3)) * 2, reads, names, d


# window END positions (read 0 starts the batch) without a count: strong runs begin and end at bits 63 / 0 / 1 of a 64-bit
# word and at the chunk edges 1024 and 2048
SEAM_WEAK_ENDS = (62, 64, 127, 192, 257, 1022, 1024, 2046, 2048)


def seams(k, seed):
    """One read of 3000 bases whose weak windows end at SEAM_WEAK_ENDS, a filler up to batch position 3072, and two reads
    behind it"""
    rng = np.random.default_rng(seed)
    g = rnd(rng, 3000)
    sample = with_holes(g, k, [e - k + 1 for e in SEAM_WEAK_ENDS])
    return sample, [g, rnd(rng, 72), g[500:500 + 3 * k], g[1000:1000 + k]]


def variants(k, seed):
    """Reads with exactly LANE_MAX and WAVE_MAX windows, one fewer and one more, a read of 5000 bases (a wave's lanes own 128
    window bits each) and one of 70 000 (a workgroup's threads own 320 each, its second wave begins near window 20 480),
    with substitutions that leave their longest strong run across those seams.  The genome is counted once: range (1, 0)."""
    rng = np.random.default_rng(seed)
    g = rnd(rng, 71000)
    reads = []
    for nw in (LANE_MAX - 1, LANE_MAX, LANE_MAX + 1, WAVE_MAX - 1, WAVE_MAX, WAVE_MAX + 1):
        s = g[100:100 + nw + k - 1]
        for p in range(40, len(s), 90 if nw < 2000 else 2900):
            s = sub(s, p)
        reads.append(s)
    s = g[:5000]
    for p in (300, 700, 1900, 2600, 3100, 4000, 4700):   # the longest run: windows 701 .. 1869, across nine lanes' slices
        s = sub(s, p)
    reads.append(s)
    s = g[:70000]
    for p in list(range(1500, 19000, 1500)) + list(range(22500, 70000, 1500)):   # the longest run: windows 18001 .. 22469
        s = sub(s, p)
    reads.append(s)
    return [g], reads


GATHER_LENS = (0, 1, 15, 16, 17, 31, 32, 33)


def alignment(k, seed):
    """For INVERT with min_strong 1 (reads without a strong window are emitted): junk reads of GATHER_LENS bases that begin at
    every batch position mod 16 and land at every output position mod 16 -- genome reads (dropped) move the first, junk
    fillers (emitted, some empty) the second -- then 40 reads of one base and 5 empty ones.  Returns (sample, reads, the
    (length, source alignment, destination alignment) triples met)."""
    rng = np.random.default_rng(seed)
    g = rnd(rng, 400)
    reads, met, P, D = [], set(), 0, 0
    for n in GATHER_LENS:
        for s in range(16):
            for d in range(16):
                x = (d - D) % 16
                reads.append(rnd(rng, x))
                P, D = P + x, D + x
                y = k + (s - P - k) % 16
                a = int(rng.integers(0, len(g) - y + 1))
                reads.append(g[a:a + y])
                P += y
                met.add((n, P % 16, D % 16))
                reads.append(rnd(rng, n))
                P, D = P + n, D + n
    reads += [rnd(rng, 1) for _ in range(40)] + [""] * 5 + [rnd(rng, 1) for _ in range(3)]
    return [g, g], reads, met


def pairs(k, seed):
    """Eight reads: the mates pass / fail in all four combinations, twice (a genome read passes min_strong 1, junk fails)"""
    rng = np.random.default_rng(seed)
    g = rnd(rng, 600)
    good = lambda: g[int(rng.integers(0, 400)):][:3 * k + int(rng.integers(0, 9))]
    bad = lambda: rnd(rng, 2 * k + 5)
    reads = []
    for _ in range(2):
        reads += [good(), good(), good(), bad(), bad(), good(), bad(), bad()]
    return [g, g], reads
