"""Test-side references for the owner partition of the multi-GPU reduce (kmc_owner_of / kmc_partition_device): the
owner function once more in plain Python integers, and a check of a whole partition result, every entry, in vectorised
numpy.  Test infrastructure only."""
import importlib

import numpy as np

M64 = (1 << 64) - 1


def owner_py(key_hi: int, key_lo: int, n_parts: int) -> int:
    """kmc_owner_of in Python integers, every product masked to 64 bits (include/kmc.h: splitmix64 finalizer of
    lo ^ hi * golden, the upper 32 bits scaled to n_parts)."""
    z = (int(key_lo) ^ ((int(key_hi) * 0x9E3779B97F4A7C15) & M64)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z = z ^ (z >> 31)
    return ((z >> 32) * int(n_parts)) >> 32


def owned(whole, n_parts: int, part: int):
    """(key_hi, key_lo, count) of the keys of a sorted table that `part` owns, in the table's order."""
    kd = importlib.import_module("k-mer-count_amd.distributed")
    m = kd.owner_np(whole.key_hi, whole.key_lo, n_parts) == part
    return whole.key_hi[m], whole.key_lo[m], whole.count[m]


def check_partition(pb, out_hi, out_lo, out_cnt, w_hi, w_lo, w_cnt, n_parts: int):
    """A kmc_partition_device result (part_begin and the three reordered arrays, on the host) against the sorted table
    (w_*) it was cut from: part_begin is the cumulative bincount of the owners, EVERY entry of part p has owner p, and
    every part, sorted, is the table's keys of that owner with their counts."""
    kd = importlib.import_module("k-mer-count_amd.distributed")
    n = int(w_lo.shape[0])
    pb = np.asarray(pb, dtype=np.int64)
    assert pb.shape == (n_parts + 1,)
    own_w = kd.owner_np(w_hi, w_lo, n_parts)
    want_pb = np.zeros(n_parts + 1, np.int64)
    want_pb[1:] = np.cumsum(np.bincount(own_w, minlength=n_parts))
    assert np.array_equal(pb, want_pb), "part_begin is not the cumulative owner count"
    assert out_lo.shape[0] == n and out_cnt.shape[0] == n and out_hi.shape[0] == n
    part_of_pos = np.repeat(np.arange(n_parts, dtype=np.int64), np.diff(pb))
    own_out = kd.owner_np(out_hi, out_lo, n_parts)
    bad = np.nonzero(own_out != part_of_pos)[0]
    assert bad.size == 0, "entry %d lies in part %d, its owner is %d (%d misplaced)" % (bad[0], part_of_pos[bad[0]], own_out[bad[0]], bad.size)
    # the order inside a part is arbitrary: sort by (part, key) and compare with the table in (owner, key) order
    got = np.lexsort((out_lo, out_hi, part_of_pos))
    want = np.argsort(own_w, kind="stable")       # (the table is sorted by key)
    assert np.array_equal(out_hi[got], w_hi[want]) and np.array_equal(out_lo[got], w_lo[want]), "a part's keys are not its owner's keys"
    assert np.array_equal(out_cnt[got], w_cnt[want]), "a count moved away from its key"
