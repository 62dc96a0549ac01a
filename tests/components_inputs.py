"""The hand-built inputs of the components tests (test_components_host.py, test_components_gpu.py): the smallest shapes at
which the kernels of kmc_components.hip.h can go wrong.  Every builder is seeded and returns a list of reads."""
import numpy as np

import bubble_inputs as bi
import clean_inputs as ci
import graph_model as gm
from clean_inputs import rnd


def ladder(k, seed, n=40):
    """a backbone of (2n + 3)k bases read three times with n substitution bubbles, one every 2k bases: 3n + 1 unitigs in a
    chain -- segment, two arms, segment, ... -- whose ids follow the key order, not the chain: a label has some 2n steps to
    travel, so the label rounds are many"""
    rng = np.random.default_rng(seed)
    s = rnd(rng, (2 * n + 3) * k)
    reads = [s] * 3
    for i in range(n):
        p = (2 * i + 2) * k
        reads.append(s[p - (k - 1):p] + bi._other(rng, s[p]) + s[p + 1:p + k])
    return reads


def islands_and_fork(k, seed, n=300):
    """n reads of 1..8 keys connected to nothing beside one fork: more than 256 unitigs (a second workgroup) and waves
    whose lanes all add to different components"""
    rng = np.random.default_rng(seed)
    reads = [rnd(rng, k + int(rng.integers(0, 8))) for _ in range(n)]
    return reads[:n // 2] + ci.fork(rng, 2 * k + 5, (4, 6))[0] + reads[n // 2:]


def comb(k, seed, n=70):
    """one component of 2n + 1 unitigs: a backbone read three times with a dead-end arm of 4 keys every 2k bases -- whole
    waves whose lanes all add to one component"""
    rng = np.random.default_rng(seed)
    s = rnd(rng, (2 * n + 2) * k)
    reads = [s] * 3
    for i in range(n):
        p = (2 * i + 2) * k
        reads.append(s[p - (k - 1):p] + bi._other(rng, s[p]) + rnd(rng, 3))
    return reads


def boundary(k, seed, n_keys):
    """components of exactly n_keys and n_keys + 1 keys -- one unconnected read each -- and a fork of k + 11 keys in three
    unitigs"""
    rng = np.random.default_rng(seed)
    return [rnd(rng, n_keys + k - 1), rnd(rng, n_keys + k)] + ci.fork(rng, 2 * k, (4, 4))[0]


def hairpin(k, seed):
    """a sequence followed by its own reverse complement: in a canonical ctx a unitig whose END end links to itself"""
    h = rnd(np.random.default_rng(seed), 2 * k)
    return [h + gm.revcomp(h)]


def two_forks(k, seed):
    """two forks that share nothing, the one with the long arms of 3k keys and the one with arms of 4 keys: which of them
    is component 0 is decided by the smallest key, not by the size"""
    rng = np.random.default_rng(seed)
    return ci.fork(rng, 2 * k + 5, (3 * k, 3 * k))[0] + ci.fork(rng, 2 * k + 5, (4, 4))[0]


def built(k, seed=0):
    """{name: reads} of every input the tests run"""
    return {"ladder": ladder(k, 1000 + seed + k), "islands_and_fork": islands_and_fork(k, 1100 + seed + k), "comb": comb(k, 1200 + seed + k),
            "boundary": boundary(k, 1300 + seed + k, k + 3), "circular": [bi.circular(k, 70 + k)] + boundary(k, 1400 + seed + k, 2 * k),
            "hairpin": hairpin(k, 1500 + seed + k) + two_forks(k, 1600 + seed + k), "two_forks": two_forks(k, 1700 + seed + k),
            "everything": bi.everything(k, 90 + k), "rounds_input": ci.rounds_input(k, 400 + k)}
