"""Inputs of the normalise tests (tests/test_normalize_host.py, tests/test_normalize_gpu.py): a table {k-mer string: count}
with seeded counts -- loaded into a ctx as (key, count) pairs, so that counts of every size occur -- and the reads that are
judged against it, with a dict of names.  CPU only; nothing here touches the library."""
import numpy as np

import graph_model as gm
from map_inputs import pack, rnd  # noqa: F401  (part of this module's interface)

# the select kernel's variants (kmc_normalize.hip.h: "#define KMC_NM_SLOTS 16", KMC_NM_WAVE_MAX = 64 * KMC_NM_SLOTS), in windows
WAVE_MAX = 1024
# windows of the plain reads: one and two, both sides of a wave's 64 lanes, both sides of the variant boundary, and a
# workgroup read whose windows are no multiple of its 256 threads
WINDOWS = (1, 2, 63, 64, 65, WAVE_MAX - 1, WAVE_MAX, WAVE_MAX + 1, 2471)
VARIANTS = ("spread", "top", "low", "ties")
BIG = (1 << 32) + 5          # the count of two keys: a depth saturates at 0xFFFFFFFF
PERMILLES = (0, 1, 499, 500, 501, 999, 1000)


def seeded_counts(rng, n, variant):
    """spread: all four bytes differ, so every digit pass decides; top / low: the counts differ in the top / the low byte alone;
    ties: three values, one of them in most windows"""
    if variant == "spread":
        return [int(x) for x in rng.integers(1, 1 << 32, n)]
    if variant == "top":
        return [(int(x) << 24) | 0xABCDEF for x in rng.integers(0, 256, n)]
    if variant == "low":
        return [0x12345600 | int(x) for x in rng.integers(0, 256, n)]
    assert variant == "ties"
    return [(7, 7, 7, 0x01000007, 0xFF000007)[int(x)] for x in rng.integers(0, 5, n)]


def kmers(s, k, canonical):
    return [gm.canon(s[j:j + k], canonical) for j in range(len(s) - k + 1)]


def table_and_reads(k, seed, canonical, variant="spread"):
    """(table, reads, {name: read index})"""
    rng = np.random.default_rng(seed)
    g = rnd(rng, 4200)
    absent = rnd(rng, k + 20)
    gone = set(kmers(absent, k, canonical))
    keys = kmers(g, k, canonical)
    table = {x: c for x, c in zip(keys, seeded_counts(rng, len(keys), variant)) if x not in gone}
    for x in keys[:2]:
        if x not in gone:
            table[x] = BIG
    names, reads = {}, []

    def add(name, s):
        names[name] = len(reads)
        reads.append(s)
    for nw in WINDOWS:
        a = int(rng.integers(2, len(g) - (nw + k - 1) + 1))
        add("w%d" % nw, g[a:a + nw + k - 1])
    add("short", g[:k - 1])
    add("empty", "")
    add("all_N", "N" * (k + 30))
    s = g[100:400]
    add("holes", s[:50] + "N" + s[51:120] + s[120:124].lower() + s[124:-1] + "N")
    add("empty2", "")
    s = g[200:1700]
    add("holes_long", s[:700] + "N" + s[701:1000] + s[1000:1003].lower() + s[1003:])
    add("absent", absent)
    add("big", g[:k + 40])
    add("empty3", "")
    return table, reads, names


def pairs(k, seed):
    """(table, reads): a deep genome A (every key 100), a shallow one B (every key 4) and junk; mates in every combination,
    then twenty (A, A) pairs so that the draw keeps some deep units and drops others.  For target 40, min_depth 2."""
    rng = np.random.default_rng(seed)
    A, B = rnd(rng, 900), rnd(rng, 900)
    table = {x: 4 for x in kmers(B, k, True)}
    table.update({x: 100 for x in kmers(A, k, True)})
    a = lambda: A[int(rng.integers(0, 700)):][:2 * k + int(rng.integers(0, 40))]
    b = lambda: B[int(rng.integers(0, 700)):][:2 * k + int(rng.integers(0, 40))]
    j = lambda: rnd(rng, 2 * k)
    reads = [a(), b(), b(), a(), b(), b(), a(), j(), j(), b(), j(), j()]
    for _ in range(20):
        reads += [a(), a()]
    return table, reads


def pairs_arrays(kmc, table):
    """the table as (key_hi, key_lo, count) arrays of uint64 for merge_pairs_device (the keys are canonical already)"""
    keys = sorted(table)
    enc = [kmc.encode_key(x, False) for x in keys]
    return (np.array([e[0] for e in enc], np.uint64), np.array([e[1] for e in enc], np.uint64), np.array([table[x] for x in keys], np.uint64))
