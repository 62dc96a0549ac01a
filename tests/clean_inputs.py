"""The hand-built inputs of the clean tests (test_clean_host.py, test_clean_gpu.py): forks whose arms compete as tips,
islands, a fork whose decision needs a 128-bit product, and the input of the rounds test.  Every fork is a random stem and
arms ``stem + base + tail`` with a different base each; an arm's unitig has len(tail) + 1 keys."""
import numpy as np

import graph_model as gm


def rnd(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def fork(rng, stem_len, tails, times=None):
    """(reads, arm strings): a stem of stem_len bases, one arm per entry of tails (its length), arm i read times[i] times"""
    stem = rnd(rng, stem_len)
    first = rng.permutation(4)
    arms = [stem + "ACGT"[first[i]] + rnd(rng, t) for i, t in enumerate(tails)]
    reads = []
    for i, a in enumerate(arms):
        reads += [a] * (times[i] if times else 1)
    return reads, arms


def five_forks(k, seed):
    """(reads, [arms of fork 1..5]): tails (4, 4) seen twice and once; (4, 6); (4, 4); (4, 4, 3k); (k - 1, k)"""
    rng = np.random.default_rng(seed)
    reads, arms = [], []
    for tails, times in (((4, 4), (2, 1)), ((4, 6), None), ((4, 4), None), ((4, 4, 3 * k), None), ((k - 1, k), None)):
        r, a = fork(rng, 2 * k + 5, tails, times)
        reads += r
        arms.append(a)
    return reads, arms


def islands(k, seed):
    """two reads connected to nothing: one of 3 keys, one of k + 1 keys"""
    rng = np.random.default_rng(seed)
    return [rnd(rng, k + 2), rnd(rng, 2 * k)]


def unitig_of(model_unitigs, arm, k, canonical):
    """the index of the unitig that holds the last k-mer of an arm"""
    key = gm.canon(arm[-k:], canonical)
    hits = [i for i, s in enumerate(model_unitigs.seqs) if any(gm.canon(s[j:j + k], canonical) == key for j in range(len(s) - k + 1))]
    assert len(hits) == 1
    return hits[0]


def wide_fork(k, canonical, seed):
    """(table, arm of 5 keys, arm of 6 keys): a fork whose arm keys' counts are rewritten so that the 6-key arm has the
    abundance ceil(2^64 / 5) + 7 and the 5-key arm floor((2^64 - 1) / 6), spread evenly over their keys.  Exactly,
    A6 * 5 > 2^64 > A5 * 6: the 6-key arm has the higher mean and stays.  Truncated to 64 bits A6 * 5 is a small number and
    the 5-key arm would stay.  The whole table sums to less than 2^64."""
    rng = np.random.default_rng(seed)
    reads, arms = fork(rng, 2 * k + 5, (4, 5))
    table = gm.count_table(reads, k, canonical)
    a6, a5 = -(-(1 << 64) // 5) + 7, ((1 << 64) - 1) // 6
    for arm, keys, total in ((arms[0], 5, a5), (arms[1], 6, a6)):
        for j in range(keys):
            x = gm.canon(arm[len(arm) - k - j:len(arm) - j], canonical)
            assert table[x] == 1
            table[x] = total // keys + (1 if j < total % keys else 0)
    assert (a6 * 5) % (1 << 64) < a5 * 6 < (1 << 64) < a6 * 5 and sum(table.values()) < (1 << 64)
    return table, arms[0], arms[1]


def rounds_input(k, seed):
    """A sequence of 6k bases seen three times with a 4-key mismatch tip in its middle, a stem of 2k bases with a twice-seen
    and a once-seen arm of 5 keys, an island of 3 keys.  One round leaves two unitigs, of 5k + 1 and of k + 6 keys."""
    rng = np.random.default_rng(seed)
    s = rnd(rng, 6 * k)
    p = 3 * k
    alt = "ACGT"[("ACGT".index(s[p]) + 1 + int(rng.integers(0, 3))) % 4]
    reads = [s] * 3 + [s[p - (k - 1):p] + alt + s[p + 1:p + 4]]
    reads += fork(rng, 2 * k, (4, 4), (2, 1))[0]
    reads.append(rnd(rng, k + 2))
    return reads
