"""The hand-built inputs of the simplify tests (test_simplify_host.py, test_simplify_gpu.py).  A bubble is a read that
repeats a stretch of a sequence with one position changed: ``s[p - (k - 1):p] + alt + s[p + 1:p + k]`` has exactly the k
k-mers that hold the changed base, so its arm leaves the sequence's path at a fork and rejoins it k keys later, beside
the true arm of k keys.  Every builder is seeded; the ones whose tests name single unitigs draw their sequence again until
no (k-1)-mer of it occurs twice, on either strand, so that the graph has no branch but the built ones even at k = 5."""
import numpy as np

import graph_model as gm
from clean_inputs import rnd


def _other(rng, *bases):
    """a base that is none of the given ones"""
    return [b for b in "ACGT" if b not in bases][int(rng.integers(0, 4 - len(set(bases))))]


def _plain(pieces, k):
    """no (k-1)-mer occurs twice among the pieces, read on either strand, and none is its own reverse complement"""
    seen = set()
    for s in pieces:
        for j in range(len(s) - k + 2):
            x = s[j:j + k - 1]
            y = gm.revcomp(x)
            if x == y or x in seen or y in seen:
                return False
            seen.add(x)
    return True


def _sub_read(s, p, k, alt):
    return s[p - (k - 1):p] + alt + s[p + 1:p + k]


def substitution(k, seed):
    """(reads, s, error read): a sequence of 6k bases read three times and one read that covers position 3k with another
    base there.  Four unitigs: 2k and 2k + 1 keys of the sequence beside the bubble, the true arm and the error arm of k keys
    each, with abundances 6k, 6k + 3, 3k and k."""
    rng = np.random.default_rng(seed)
    p = 3 * k
    while True:
        s = rnd(rng, 6 * k)
        alt = _other(rng, s[p])
        err = _sub_read(s, p, k, alt)
        if _plain([s, s[p - (k - 2):p] + alt + s[p + 1:p + k - 1]], k):   # (the second piece: the (k-1)-mers that hold alt)
            return [s] * 3 + [err], s, err


def three_arms(k, seed):
    """(reads, s, [error read seen once, error read seen twice]): position 3k read with three different bases"""
    rng = np.random.default_rng(seed)
    s = rnd(rng, 6 * k)
    p = 3 * k
    a1 = _other(rng, s[p])
    a2 = _other(rng, s[p], a1)
    e1, e2 = _sub_read(s, p, k, a1), _sub_read(s, p, k, a2)
    return [s] * 3 + [e1, e2, e2], s, [e1, e2]


def arms_k_and_k_plus_1(k, seed):
    """(reads, s, arm of k keys, arm of k + 1 keys): a sequence of 12k bases read three times, one substitution at 3k (an arm
    of k keys beside a true arm of k keys) and two adjacent ones at 8k (an arm of k + 1 keys beside a true arm of k + 1)"""
    rng = np.random.default_rng(seed)
    s = rnd(rng, 12 * k)
    p, q = 3 * k, 8 * k
    e1 = _sub_read(s, p, k, _other(rng, s[p]))
    e2 = s[q - (k - 1):q] + _other(rng, s[q]) + _other(rng, s[q + 1]) + s[q + 2:q + 1 + k]
    return [s] * 3 + [e1, e2], s, e1, e2


def insertion(rng, s, p, k):
    """a read with one base inserted before s[p]: an arm of k keys beside a true arm of k - 1 keys"""
    return s[p - (k - 1):p] + _other(rng, s[p], s[p - 1]) + s[p:p + k - 1]


def decided_pairs(k, seed):
    """(reads, [(error read, level that decides)]): three sequences of 6k bases, each with one bubble at 3k -- read three
    times beside a substitution seen once (the mean abundance decides); read once beside an insertion seen once (equal
    means, k - 1 keys against k: the keys decide); read once beside a substitution seen once (equal in both: the id)"""
    rng = np.random.default_rng(seed)
    s1, s2, s3 = (rnd(rng, 6 * k) for _ in range(3))
    p = 3 * k
    e1 = _sub_read(s1, p, k, _other(rng, s1[p]))
    e2 = insertion(rng, s2, p, k)
    e3 = _sub_read(s3, p, k, _other(rng, s3[p]))
    return [s1] * 3 + [e1, s2, e2, s3, e3], [(e1, "abundance"), (e2, "keys"), (e3, "id")]


def wide_bubble(k, canonical, seed):
    """(table, true arm's k-mers, inserted arm's k-mers): an insertion bubble, arms of k - 1 and k keys, whose arm keys' counts
    are rewritten so that the k-key arm has the abundance ceil(2^64 / (k - 1)) + 7 and the (k - 1)-key arm
    floor((2^64 - 1) / k), spread evenly over their keys.  Exactly, A_k * (k - 1) > 2^64 > A_(k-1) * k: the k-key arm has the
    higher mean and stays.  Truncated to 64 bits A_k * (k - 1) is a small number and the (k - 1)-key arm would stay."""
    rng = np.random.default_rng(seed)
    p = 3 * k
    while True:
        s = rnd(rng, 6 * k)
        e = insertion(rng, s, p, k)
        if _plain([s, e[1:2 * k - 2]], k):                                                 # (the (k-1)-mers that hold the inserted base)
            break
    table = gm.count_table([s, e], k, canonical)
    true_arm = [gm.canon(s[j:j + k], canonical) for j in range(p - (k - 1), p)]            # the k-mers that hold s[p - 1] and s[p]
    ins_arm = [gm.canon(e[j:j + k], canonical) for j in range(k)]                          # the k-mers that hold the inserted base
    a_long, a_short = -(-(1 << 64) // (k - 1)) + 7, ((1 << 64) - 1) // k
    for keys, total in ((true_arm, a_short), (ins_arm, a_long)):
        assert len(set(keys)) == len(keys)
        for j, x in enumerate(keys):
            assert table[x] == 1
            table[x] = total // len(keys) + (1 if j < total % len(keys) else 0)
    assert (a_long * (k - 1)) % (1 << 64) < a_short * k < (1 << 64) < a_long * (k - 1) and sum(table.values()) < (1 << 64)
    return table, true_arm, ins_arm


def tip_and_bubble(k, seed):
    """(reads, error read, tip read): the fork at 3k has three ways on: the true arm, a substitution's arm and a dead end of
    4 keys"""
    rng = np.random.default_rng(seed)
    s = rnd(rng, 6 * k)
    p = 3 * k
    a1 = _other(rng, s[p])
    a2 = _other(rng, s[p], a1)
    err = _sub_read(s, p, k, a1)
    tip = s[p - (k - 1):p] + a2 + rnd(rng, 3)
    return [s] * 3 + [err, tip], err, tip


def circular(k, seed):
    """a read that goes once round a cycle of 2k keys: one circular unitig"""
    c = rnd(np.random.default_rng(seed), 2 * k)
    return c + c[:k - 1]


def same_end(k, seed):
    """(two reads, u): x + u and x + revcomp(u).  In a canonical ctx the k-mers of u and the two junctions are one unitig
    whose START and END end both reach the END end of x's unitig (p == q); in a forward ctx it is a fork with two dead ends."""
    rng = np.random.default_rng(seed)
    x, u = rnd(rng, 2 * k), rnd(rng, k + 3)
    return [x + u, x + gm.revcomp(u)], u


def field(k, seed, n=320):
    """(reads, error reads): n independent bubbles, each a sequence of 3k bases read twice and a substitution read at 3k / 2
    + k / 2: 4n unitigs, n of them to pop"""
    rng = np.random.default_rng(seed)
    reads, errs = [], []
    for _ in range(n):
        s = rnd(rng, 3 * k)
        p = k + k // 2
        e = _sub_read(s, p, k, _other(rng, s[p]))
        reads += [s, s, e]
        errs.append(e)
    return reads, errs


def everything(k, seed):
    """the reads of all the small builders in one table"""
    return (substitution(k, seed)[0] + three_arms(k, seed + 1)[0] + arms_k_and_k_plus_1(k, seed + 2)[0] + decided_pairs(k, seed + 3)[0] +
            tip_and_bubble(k, seed + 4)[0] + [circular(k, seed + 5)] + same_end(k, seed + 6)[0])


def unitig_with(model_unitigs, kmer, k, canonical):
    """the index of the unitig that holds a k-mer"""
    key = gm.canon(kmer, canonical)
    hits = [i for i, s in enumerate(model_unitigs.seqs) if any(gm.canon(s[j:j + k], canonical) == key for j in range(len(s) - k + 1))]
    assert len(hits) == 1
    return hits[0]
