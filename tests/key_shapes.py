"""Adversarial key multisets for the sort and hash paths, injected through reads of exactly k bases.

In forward mode (canonical=False) a read of exactly k bases has one window, so a batch of such reads is an arbitrary
multiset of packed keys.  This module builds such multisets with the structure the MSD sort (csrc/kmc_msd.hip.h) and the
count table (csrc/kmc_device.hip.h: gtable_add) branch on -- equal keys, one hot key, long shared prefixes, keys that
differ in a few low bits, children at the leaf-merging edges, skewed leaves, the "staircase" that maximises the terminal
list -- decodes them to reads, and computes the table they must give with numpy alone (expected_table: np.lexsort and a
run-length).  Pure numpy: nothing here calls the library, and nothing of it needs a GPU.

A key is (hi, lo), two uint64 words, 2 bits per base, MSB first, A0 C1 G2 T3 (include/kmc.h); hi is zero for k <= 32.
Every generator is seeded and deterministic and returns (hi, lo) or (hi, lo, weights).
"""
import numpy as np

U64 = np.uint64
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
# byte -> its four bases, most significant pair first
_BYTE_BASES = _ACGT[(np.arange(256)[:, None] >> np.array([6, 4, 2, 0])[None, :]) & 3].astype(np.uint8)


# ---- 128-bit helpers on (hi, lo) uint64 arrays --------------------------------------------------------------------
def _u(x, n=None):
    a = np.asarray(x, dtype=U64)
    return np.full(n, a, dtype=U64) if (a.ndim == 0 and n is not None) else a


def key_mask(k):
    """(hi, lo) Python ints masking a k-mer's 2k bits."""
    m = (1 << (2 * k)) - 1
    return m >> 64, m & ((1 << 64) - 1)


def put_field(hi, lo, value, pos, width):
    """OR `value` (uint64 array or scalar, below 2^width, width <= 64) into bits [pos, pos + width) of the keys, in place."""
    if width <= 0:
        return
    v = _u(value) & U64((1 << width) - 1 if width < 64 else 0xFFFFFFFFFFFFFFFF)
    if pos >= 64:
        hi |= v << U64(pos - 64)
    else:
        lo |= v << U64(pos)
        if pos + width > 64 and pos > 0:
            hi |= v >> U64(64 - pos)


def random_bits(rng, n, bits):
    """n uniformly random `bits`-bit values as (hi, lo)."""
    lo = rng.integers(0, 1 << min(bits, 64), n, dtype=U64, endpoint=False) if bits > 0 else np.zeros(n, U64)
    hi = rng.integers(0, 1 << (bits - 64), n, dtype=U64, endpoint=False) if bits > 64 else np.zeros(n, U64)
    return hi, lo


def from_ints(values):
    """Python ints -> (hi, lo)."""
    hi = np.array([v >> 64 for v in values], dtype=U64)
    lo = np.array([v & ((1 << 64) - 1) for v in values], dtype=U64)
    return hi, lo


def to_ints(hi, lo):
    return [(int(h) << 64) | int(l) for h, l in zip(hi, lo)]


def key_less(ah, al, bh, bl):
    return (ah < bh) | ((ah == bh) & (al < bl))


def _shuffle(rng, *arrays):
    p = rng.permutation(arrays[0].shape[0])
    return tuple(a[p] for a in arrays)


# ---- keys -> reads ------------------------------------------------------------------------------------------------
def decode_keys(hi, lo, k):
    """(n, k) uint8 ASCII matrix of the keys, MSB first."""
    hi, lo = _u(hi), _u(lo)
    n = lo.shape[0]
    nbytes = (2 * k + 7) // 8
    pad = nbytes * 8 - 2 * k            # left-align the key on a byte boundary: 0, 2, 4 or 6 bits
    if pad:
        hi = (hi << U64(pad)) | (lo >> U64(64 - pad))
        lo = lo << U64(pad)
    be = np.empty((n, 16), dtype=np.uint8)
    be[:, :8] = hi.astype(">u8").view(np.uint8).reshape(n, 8)
    be[:, 8:] = lo.astype(">u8").view(np.uint8).reshape(n, 8)
    return _BYTE_BASES[be[:, 16 - nbytes:]].reshape(n, 4 * nbytes)[:, :k]


def reads_from_keys(key_hi, key_lo, k):
    """(bases, offsets): every key as one read of exactly k bases."""
    n = _u(key_lo).shape[0]
    bases = np.ascontiguousarray(decode_keys(key_hi, key_lo, k)).reshape(-1)
    return bases, np.arange(n + 1, dtype=U64) * U64(k)


def lr_reads_from_halves(L, R):
    """(bases, offsets) for KMC_MODE_LR: one read of 80 bases per (L, R) pair of 27-mers (one-word keys).  Such a read has
    ONE chunk, L = [0, 27) and R = [53, 80); the gap is filled with A."""
    L, R = _u(L), _u(R)
    n = L.shape[0]
    z = np.zeros(n, U64)
    reads = np.full((n, 80), ord("A"), dtype=np.uint8)
    reads[:, :27] = decode_keys(z, L, 27)
    reads[:, 53:] = decode_keys(z, R, 27)
    return reads.reshape(-1), np.arange(n + 1, dtype=U64) * U64(80)


def lr_keys(L, R):
    """The 54-mer key of an (L, R) pair: L's bases then R's."""
    L, R = _u(L), _u(R)
    hi = np.zeros(L.shape[0], U64)
    lo = R.copy()
    put_field(hi, lo, L, 54, 54)
    return hi, lo


# ---- the reference --------------------------------------------------------------------------------------------------
def expected_table(key_hi, key_lo, weights=None):
    """Sorted distinct keys and their summed counts (weights, or one per key): (hi, lo, count), all uint64."""
    hi, lo = _u(key_hi), _u(key_lo)
    n = lo.shape[0]
    if n == 0:
        z = np.zeros(0, U64)
        return z, z.copy(), z.copy()
    order = np.lexsort((lo, hi))
    hi, lo = hi[order], lo[order]
    head = np.empty(n, dtype=bool)
    head[0] = True
    head[1:] = (hi[1:] != hi[:-1]) | (lo[1:] != lo[:-1])
    starts = np.flatnonzero(head)
    if weights is None:
        cnt = np.diff(np.append(starts, n)).astype(U64)
    else:
        cnt = np.add.reduceat(_u(weights)[order], starts).astype(U64)
    return hi[starts], lo[starts], cnt


def revcomp(hi, lo, k):
    """Reverse complement of every key."""
    hi, lo = _u(hi), _u(lo)
    n = lo.shape[0]
    oh, ol = np.zeros(n, U64), np.zeros(n, U64)
    for i in range(k):                        # base i counted from the last one goes to place i counted from the first
        s = 2 * i
        b = ((lo >> U64(s)) if s < 64 else (hi >> U64(s - 64))) & U64(3)
        put_field(oh, ol, U64(3) - b, 2 * (k - 1 - i), 2)
    return oh, ol


def canonical_keys(hi, lo, k):
    """min(key, revcomp(key)) per key."""
    hi, lo = _u(hi), _u(lo)
    rh, rl = revcomp(hi, lo, k)
    take = key_less(rh, rl, hi, lo)
    return np.where(take, rh, hi), np.where(take, rl, lo)


# ---- shapes ---------------------------------------------------------------------------------------------------------
def one_key(k, n, seed=1):
    """Shape 1: one key, n times."""
    rng = np.random.default_rng(seed)
    h, l = random_bits(rng, 1, 2 * k)
    return np.repeat(h, n), np.repeat(l, n)


def heavy_plus_singletons(k, n_heavy, n_single, where="middle", seed=2):
    """Shape 2: n_heavy copies of one key among n_single random keys; the heavy key is the smallest possible key (poly-A),
    the largest (poly-T) or the median of the random ones."""
    rng = np.random.default_rng(seed)
    sh, sl = random_bits(rng, n_single, 2 * k)
    if where == "smallest":
        kh, kl = 0, 0
    elif where == "largest":
        kh, kl = key_mask(k)
    else:
        o = np.lexsort((sl, sh))[n_single // 2]
        kh, kl = int(sh[o]), int(sl[o])
    hi = np.concatenate([sh, np.full(n_heavy, kh, dtype=U64)])
    lo = np.concatenate([sl, np.full(n_heavy, kl, dtype=U64)])
    return _shuffle(rng, hi, lo)


def zipf_heavy(k, n_top, n_single, n_keys=10, seed=3):
    """Shape 2, Zipf-like: n_keys heavy keys of n_top, n_top / 2, n_top / 3 ... copies among n_single random keys."""
    rng = np.random.default_rng(seed)
    sh, sl = random_bits(rng, n_single, 2 * k)
    kh, kl = random_bits(rng, n_keys, 2 * k)
    reps = np.array([max(1, n_top // (i + 1)) for i in range(n_keys)])
    hi = np.concatenate([sh, np.repeat(kh, reps)])
    lo = np.concatenate([sl, np.repeat(kl, reps)])
    return _shuffle(rng, hi, lo)


def shared_prefix(k, n, p, seed=4):
    """Shape 3: all keys agree in their top p bits (a random prefix), the rest is random."""
    kb = 2 * k
    assert 0 <= p < kb
    rng = np.random.default_rng(seed)
    hi, lo = random_bits(rng, n, kb - p)
    ph, pl = random_bits(rng, 1, p)
    top_h, top_l = np.zeros(1, U64), np.zeros(1, U64)
    # the prefix, shifted up by kb - p bits, one word at a time
    put_field(top_h, top_l, pl, kb - p, min(p, 64))
    if p > 64:
        put_field(top_h, top_l, ph, kb - p + 64, p - 64)
    return hi | top_h[0], lo | top_l[0]


def low_bits(k, n, b, dense=True, seed=5):
    """Shape 4: n keys that differ in their lowest b bits only.  dense: all 2^b values are drawn from; sparse: a sixteenth
    of them (two at least)."""
    kb = 2 * k
    assert b < kb and b <= 32
    rng = np.random.default_rng(seed)
    ph, pl = random_bits(rng, 1, kb)
    pl = pl & ~U64((1 << b) - 1)
    if dense:
        low = rng.integers(0, 1 << b, n, dtype=U64)
        low[:2] = (0, (1 << b) - 1)           # bit b - 1 really differs
    else:
        vals = rng.choice(1 << b, size=max(2, (1 << b) // 16), replace=False).astype(U64)
        vals[:2] = (0, (1 << b) - 1)
        low = vals[rng.integers(0, vals.shape[0], n)]
        low[:2] = vals[:2]
    return np.full(n, ph[0], dtype=U64), pl[0] | low


def by_digit(k, sizes, seed=6, level_bits=10):
    """Shape 5: level-0 children of chosen sizes.  sizes[d] keys get d as their top `level_bits` bits; the rest is random."""
    kb = 2 * k
    assert kb > level_bits
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, dtype=np.int64)
    digit = np.repeat(np.arange(sizes.shape[0], dtype=U64), sizes)
    hi, lo = random_bits(rng, digit.shape[0], kb - level_bits)
    put_field(hi, lo, digit, kb - level_bits, level_bits)
    return _shuffle(rng, hi, lo)


def leaf_edge_sizes(leaf_cap):
    """Shape 5: name -> sizes[1024] of the level-0 children."""
    nd = 1024
    out = {}
    out["all_leaf_cap"] = np.full(nd, leaf_cap)
    a = np.ones(nd, dtype=np.int64); a[1::2] = leaf_cap
    out["alt_1_cap"] = a
    a = np.ones(nd, dtype=np.int64); a[1::2] = leaf_cap + 1
    out["alt_1_cap_plus_1"] = a
    # runs of eight children that sum to exactly leaf_cap, and to one more
    a = np.full(nd, leaf_cap // 8)
    out["runs_sum_cap"] = a.copy()
    a[7::8] += 1
    out["runs_sum_cap_plus_1"] = a
    a = np.zeros(nd, dtype=np.int64)
    a[[0, 63, 64, 127, 128, 1023]] = [3, leaf_cap, leaf_cap + 1, 1, 2 * leaf_cap, 5]
    out["wave_boundaries"] = a
    return out


def sub_bucket_skew(k, variant, leaf_cap=2048, seed=7):
    """Shape 6: one leaf (at most leaf_cap keys, one level-0 digit) whose 512 sub-buckets are filled unevenly.
      one_bucket   two keys span the leaf's range, all others are distinct and sit within its first 1/512
      equal_33     33 copies of one key among random ones
      equal_most   leaf_cap - 8 copies of one key plus eight random ones
      equal_2048   2048 copies of one key alone in their digit, eight random keys in the next digit: a leaf of 2048 keys
                   that holds nothing else (leaves of 1024 keys: a big child of equal keys)
      below_bits   two far keys, all others differ in their lowest four bits only (16 values, many copies)"""
    kb = 2 * k
    assert kb >= 30
    rng = np.random.default_rng(seed)
    free = kb - 10                                  # bits below the level-0 digit
    top = U64(rng.integers(0, 1024))

    def finish(h, l):
        put_field(h, l, top, free, 10)
        return _shuffle(rng, h, l)

    if variant == "one_bucket":
        n = leaf_cap - 2
        h, l = np.zeros(n + 2, U64), np.zeros(n + 2, U64)
        l[:n] = rng.choice(1 << min(free - 9, 20), size=n, replace=False).astype(U64)   # within the first sub-bucket
        emax = (1 << free) - 1                      # the largest key of the digit
        eh, el = [U64(emax >> 64)], [U64(emax & ((1 << 64) - 1))]
        h[n + 1], l[n + 1] = eh[0], el[0]           # (key n stays 0: the leaf's smallest)
        return finish(h, l)
    if variant in ("equal_33", "equal_most"):
        n_eq = 33 if variant == "equal_33" else leaf_cap - 8
        n_rand = leaf_cap - 100 - n_eq if variant == "equal_33" else 8
        h, l = random_bits(rng, n_rand + 1, free)
        h = np.concatenate([h, np.repeat(h[-1:], n_eq - 1)])
        l = np.concatenate([l, np.repeat(l[-1:], n_eq - 1)])
        return finish(h, l)
    if variant == "equal_2048":
        h, l = random_bits(rng, 1, free)
        h, l = np.repeat(h, 2048), np.repeat(l, 2048)
        put_field(h, l, top, free, 10)
        oh, ol = random_bits(rng, 8, free)
        put_field(oh, ol, (top + U64(1)) % U64(1024), free, 10)
        return _shuffle(rng, np.concatenate([h, oh]), np.concatenate([l, ol]))
    if variant == "below_bits":
        n = leaf_cap - 2
        bh, bl = random_bits(rng, 1, free - 1)
        h = np.full(n + 2, bh[0], dtype=U64)
        l = np.full(n + 2, bl[0] & ~U64(15), dtype=U64)
        l[:n] |= rng.integers(0, 16, n, dtype=U64)
        h[n], l[n] = 0, 0
        put_field(h[n + 1:], l[n + 1:], U64(1), free - 1, 1)
        h[n + 1] |= bh[0]; l[n + 1] |= bl[0]
        return finish(h, l)
    raise ValueError(variant)


def staircase_levels(k):
    """The levels of the MSD sort (ten bits each, from the top) at which a staircase cluster sheds keys: levels 2, 3, ...
    whose digit lies wholly above the core's twelve low bits."""
    kb = 2 * k
    return [j for j in range(2, kb // 10 + 1) if kb - 10 * (j + 1) >= 12]


def staircase(k, n_clusters, core, seed=8, first_cluster=0, of_clusters=None):
    """Shape 7: the input that maximises the sort's terminal list.  n_clusters clusters; the cluster id sits in the top 20
    bits (spread evenly over them), so the first two levels of the sort separate the clusters.  At every later level whose
    digit lies above bit 12 the cluster's core -- `core` distinct keys that differ in their lowest 12 bits only -- sits in
    digit 512, and the cluster has exactly ONE more key in a lower digit and ONE in a higher digit of that level: the big
    child in the middle closes the group of small children before it, so every such level costs two one-key terminals.
    k = 63 has nine such levels (18 terminals) and the core ends in two leaves: 20 terminals per cluster of core + 18 keys.
    first_cluster / of_clusters: clusters [first_cluster, first_cluster + n_clusters) of an input of of_clusters, for feeding
    a large staircase in pieces.  All keys are distinct."""
    kb = 2 * k
    levels = staircase_levels(k)
    assert kb >= 42 and levels and core <= 4096
    total = of_clusters or n_clusters
    assert total <= (1 << 20)
    rng = np.random.default_rng([seed, first_cluster])
    per = core + 2 * len(levels)
    n = n_clusters * per
    hi, lo = np.zeros(n, U64), np.zeros(n, U64)
    cid = (np.arange(first_cluster, first_cluster + n_clusters, dtype=U64) * U64((1 << 20) // total))
    put_field(hi, lo, np.repeat(cid, per), kb - 20, 20)
    for j in levels:                                  # everybody starts in the middle digit of every shedding level
        put_field(hi, lo, U64(512), kb - 10 * (j + 1), 10)
    H, Lo = hi.reshape(n_clusters, per), lo.reshape(n_clusters, per)
    # the core: a fixed set of `core` low words, moved by a per-cluster xor (which keeps them distinct)
    base = rng.permutation(4096)[:core].astype(U64)
    Lo[:, :core] |= base[None, :] ^ rng.integers(0, 4096, (n_clusters, 1), dtype=U64)
    for i, j in enumerate(levels):
        pos = kb - 10 * (j + 1)                        # the level's digit is bits [pos, pos + 10)
        for side, col in ((0, core + 2 * i), (1, core + 2 * i + 1)):
            d = rng.integers(0, 512, n_clusters, dtype=U64) if side == 0 else rng.integers(513, 1024, n_clusters, dtype=U64)
            h1, l1 = np.ascontiguousarray(H[:, col]), np.ascontiguousarray(Lo[:, col])
            # clear the middle digit of this level and everything below it, then the shed digit and random bits below
            mh, ml = key_mask(k)
            keep = ((mh << 64) | ml) & ~((1 << (pos + 10)) - 1)
            h1 &= U64(keep >> 64); l1 &= U64(keep & ((1 << 64) - 1))
            put_field(h1, l1, d, pos, 10)
            rh, rl = random_bits(rng, n_clusters, pos)
            h1 |= rh; l1 |= rl
            H[:, col], Lo[:, col] = h1, l1
    return _shuffle(rng, hi, lo)


def arithmetic(k, n, stride, start=0):
    """Shape 8: start, start + stride, start + 2 stride ... (n keys, modulo 4^k)."""
    mh, ml = key_mask(k)
    m = (mh << 64) | ml
    if start + stride * n < (1 << 63):
        lo = U64(start) + np.arange(n, dtype=U64) * U64(stride)
        return np.zeros(n, U64), lo & U64(ml)
    v = (np.arange(n, dtype=object) * stride + start) & m
    return (v >> 64).astype(U64), (v & ((1 << 64) - 1)).astype(U64)


def one_word_differs(k, n, which, seed=9):
    """Shape 8 (k >= 33): keys equal in the low word and different only in the high word (which='high'), or the reverse."""
    assert k >= 33
    rng = np.random.default_rng(seed)
    hi, lo = random_bits(rng, n, 2 * k)
    if which == "high":
        lo[:] = lo[0]
    else:
        hi[:] = hi[0]
    return hi, lo


def weights_for(n, seed=10, big=False):
    """Seeded weights: mostly small, every 7th above 2^32; big=True makes the sum exceed 2^40."""
    rng = np.random.default_rng(seed)
    w = rng.integers(1, 1000, n, dtype=U64)
    w[::7] += U64(1 << 32) + rng.integers(0, 1 << 20, w[::7].shape[0], dtype=U64)
    if big:
        w[::1000] += U64(1 << 40)
    return w
