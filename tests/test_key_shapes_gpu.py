"""The sort path (csrc/kmc_msd.hip.h) and the count table (csrc/kmc_device.hip.h) on adversarial key shapes.

Every other counting test feeds random reads, which fill the top digits of the key space evenly.  The MSD sort classifies
every segment by what its keys look like (all equal, one digit, few low bits, children around the leaf size, skewed leaves)
and sizes its lists from the key count; the table probes linearly.  Here the keys are built to hit each of those branches
(tests/key_shapes.py), injected as reads of exactly k bases in forward mode or as (key, weight) pairs, and the exported
table must equal key_shapes.expected_table -- numpy's lexsort and a run-length -- key for key and count for count.

Cost (one MI355X, one session): 85 s for this file (49 cases; the two 32,000-cluster staircases take 26 s and 11 s of
it).  The rest of the `-m gpu` suite did not finish within the 600 s it was given in that session (178 of its tests had
passed by then), so the whole suite takes more than 685 s with this file, of which this file is at most an eighth.
"""
import numpy as np
import pytest

import key_shapes as ks

pytestmark = pytest.mark.gpu

BATCH = 4_000_000   # keys per add_batch call of the large cases (an ALGO_SORT ctx sorts what it has accumulated as one pass)


def _eq(t, exp):
    eh, el, ec = exp
    return (t.n_distinct == el.shape[0] and np.array_equal(t.key_hi, eh) and np.array_equal(t.key_lo, el)
            and np.array_equal(t.count, ec))


def _feed(kc, k, hi, lo):
    for a in range(0, lo.shape[0], BATCH):
        kc.add_batch(*ks.reads_from_keys(hi[a:a + BATCH], lo[a:a + BATCH], k))


def _check_sort(kmc, k, hi, lo, what, others=None, canonical=False):
    """The keys through ALGO_SORT against expected_table; with at most a million keys (or others=True) through the other
    paths as well.  Returns the expected table."""
    n = lo.shape[0]
    if canonical:
        want = ks.expected_table(*ks.canonical_keys(hi, lo, k))
    else:
        want = ks.expected_table(hi, lo)
    with kmc.KmerCounter(k=k, canonical=canonical, algo=kmc.ALGO_SORT) as kc:
        _feed(kc, k, hi, lo)
        t = kc.export()
        assert kc.stats().algo_last == kmc.ALGO_SORT, what
        assert _eq(t, want), (what, "sort")
        assert t.n_total == n, what
    if others if others is not None else n <= 1_000_000:
        bases, offs = ks.reads_from_keys(hi, lo, k)
        for algo in (kmc.ALGO_STREAM, kmc.ALGO_WALK, kmc.ALGO_AUTO):
            with kmc.KmerCounter(k=k, canonical=canonical, algo=algo) as kc:
                kc.add_batch(bases, offs)
                t = kc.export()
                assert _eq(t, want), (what, "algo", algo)
                assert t.n_total == n, (what, algo)
    return want


def _check_downstream(kc, k, want, seed):
    """histogram() and query() of the finalized ctx against the expected table: present keys (a sample and both ends)
    and absent ones (neighbours of present keys, random keys)."""
    eh, el, ec = want
    n = el.shape[0]
    nb = 1001
    h = kc.histogram(nb)
    wh = np.bincount(np.minimum(ec, np.uint64(nb - 1)).astype(np.int64), minlength=nb).astype(np.uint64)
    assert np.array_equal(h, wh)
    rng = np.random.default_rng(seed)
    idx = np.unique(np.concatenate([rng.integers(0, n, 5000), [0, n - 1, int(np.argmax(ec))]]))
    got = kc.query(el[idx], eh[idx] if k > 31 else None)
    assert np.array_equal(got, ec[idx])
    # absent: key + 1 where that is not the next key, and random keys that are not in the table
    present = set(ks.to_ints(eh, el)) if n <= 2_000_000 else None
    ah, al = ks.random_bits(rng, 5000, 2 * k)
    nl = el[idx] + np.uint64(1)
    nh = eh[idx] + (nl == 0).astype(np.uint64)
    ah, al = np.concatenate([ah, nh]), np.concatenate([al, nl])
    mh, ml = ks.key_mask(k)
    ok = (ah < np.uint64(mh)) | ((ah == np.uint64(mh)) & (al <= np.uint64(ml)))   # (key + 1 may leave the key space)
    ah, al = ah[ok], al[ok]
    # expected counts by binary search in the expected table (structured compare on (hi, lo))
    ekey = np.empty(n, dtype=[("h", np.uint64), ("l", np.uint64)]); ekey["h"], ekey["l"] = eh, el
    akey = np.empty(al.shape[0], dtype=ekey.dtype); akey["h"], akey["l"] = ah, al
    pos = np.searchsorted(ekey, akey)
    pos_c = np.minimum(pos, n - 1)
    hit = (pos < n) & (ekey["h"][pos_c] == ah) & (ekey["l"][pos_c] == al)
    exp = np.where(hit, ec[pos_c], np.uint64(0))
    if present is not None:
        assert [x in present for x in ks.to_ints(ah, al)] == hit.tolist()
    assert (~hit).sum() >= 1000
    got = kc.query(al, ah if k > 31 else None)
    assert np.array_equal(got, exp)


# ---- shape 1: one key, n times --------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [16, 31, 32, 33, 63])
def test_one_key(kmc, k):
    """All keys equal: a kind-1 terminal at level 0, one pair, n - 1 duplicates in n_dups (the gather pass)."""
    for n in (1, 2, 1024, 1025, 2048, 2049, 65536, 65537) + ((5_000_000,) if k in (31, 63) else ()):
        hi, lo = ks.one_key(k, n, seed=n)
        want = _check_sort(kmc, k, hi, lo, ("one_key", k, n), others=n <= 65537)
        assert want[1].shape[0] == 1 and int(want[2][0]) == n


# ---- shape 2: one heavy key plus singletons -------------------------------------------------------------------------
@pytest.mark.parametrize("k,scale", [(31, 1), (63, 1), (21, 16), (32, 16), (33, 16)])
def test_heavy_key_among_singletons(kmc, k, scale):
    """4 M copies of one key among 1 M random keys (a sixteenth of that for the k that also run through the table
    paths): the heavy key smallest, largest, in the middle; ten heavy keys of Zipf-like sizes.  A downstream call
    sees the same table."""
    n_heavy, n_single = 4_000_000 // scale, 1_000_000 // scale
    for where in ("smallest", "largest", "middle"):
        hi, lo = ks.heavy_plus_singletons(k, n_heavy, n_single, where)
        want = _check_sort(kmc, k, hi, lo, ("heavy", k, where))
        assert int(want[2].max()) >= n_heavy
    hi, lo = ks.zipf_heavy(k, n_heavy // 2, n_single)
    want = ks.expected_table(hi, lo)
    with kmc.KmerCounter(k=k, canonical=False, algo=kmc.ALGO_SORT) as kc:
        _feed(kc, k, hi, lo)
        assert _eq(kc.export(), want) and kc.stats().algo_last == kmc.ALGO_SORT
        _check_downstream(kc, k, want, seed=k)
    if scale > 1:
        _check_sort(kmc, k, hi, lo, ("zipf", k))


# ---- shape 3: shared long prefix ------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 31, 32, 33, 63])
def test_shared_prefix(kmc, k):
    """All keys agree in their top p bits: segments that are not moved and jump to the first differing bit, for two-word
    keys across the word boundary (p = 61, 64) and deep into the low word (p = 100, 120)."""
    for p in (9, 10, 11, 20, 40, 61, 64, 100, 120):
        if p >= 2 * k - 1:
            continue
        hi, lo = ks.shared_prefix(k, 300_000, p, seed=p)
        _check_sort(kmc, k, hi, lo, ("prefix", k, p))


# ---- shape 4: few low bits differ -----------------------------------------------------------------------------------
def _low_bit_clusters(k, n, b, seed):
    """Four spans that differ in bits [14, 16) and, inside a span, in the lowest b bits only: after the prefix jump the
    spans are big children with few bits left (kind 2 through a big child, not through a segment that is not moved)."""
    rng = np.random.default_rng(seed)
    ph, pl = ks.random_bits(rng, 1, 2 * k)
    lo = (pl[0] & ~np.uint64(0xFFFF)) | (rng.integers(0, 4, n, dtype=np.uint64) << np.uint64(14)) | rng.integers(0, 1 << b, n, dtype=np.uint64)
    return np.full(n, ph[0], dtype=np.uint64), lo


@pytest.mark.parametrize("k", [16, 31, 32, 33, 63])
def test_few_low_bits_differ(kmc, k):
    """More keys than a leaf holds that differ in their lowest b bits only, b on both sides of KMC_MSD_CNT_BITS = 14:
    counted spans (kind 2) up to 14 bits, further levels and leaves above."""
    for b in (1, 6, 13, 14, 15, 16):
        for dense in (True, False):
            hi, lo = ks.low_bits(k, 200_000, b, dense, seed=b)
            want = _check_sort(kmc, k, hi, lo, ("low_bits", k, b, dense))
            assert want[1].shape[0] <= (1 << b)
    for b in (6, 10, 13):
        hi, lo = _low_bit_clusters(k, 300_000, b, seed=b)
        _check_sort(kmc, k, hi, lo, ("low_bit_clusters", k, b))


# ---- shape 5: leaf merging edges ------------------------------------------------------------------------------------
def _sort_on_one_ctx(kmc, k, leaf_cap, cases, others=True):
    """Every case through one ALGO_SORT ctx, a reset between.  Two-word keys have leaves of 1024 keys once an unweighted
    sort of at least 2^20 keys on the ctx has collapsed its keys more than fourfold (msd_sort_to_run: msd_dup_heavy;
    kmc_reset keeps the flag, only forgetting the ctx's history clears it): for leaf_cap = 1024 that sort -- 2^20 + 4096
    copies of one key -- runs first, on the same ctx, before every case.  No call reports the leaf size of a sort, so the
    flag's lifetime is what the smaller leaves rest on here, as in test_two_word_sort_with_both_leaf_sizes."""
    assert leaf_cap == 2048 or (leaf_cap == 1024 and k > 31)
    collapse = ks.reads_from_keys(*ks.one_key(k, (1 << 20) + 4096), k) if leaf_cap == 1024 else None
    with kmc.KmerCounter(k=k, canonical=False, algo=kmc.ALGO_SORT) as kc:
        for name, (hi, lo) in cases:
            want = ks.expected_table(hi, lo)
            kc.reset()
            if collapse is not None:
                kc.add_batch(*collapse)
                assert kc.export().n_distinct == 1
                kc.reset()
            _feed(kc, k, hi, lo)
            t = kc.export()
            assert kc.stats().algo_last == kmc.ALGO_SORT
            assert _eq(t, want) and t.n_total == lo.shape[0], (name, k, leaf_cap)
            if others and lo.shape[0] <= 1_000_000 and leaf_cap == 2048:
                _check_sort(kmc, k, hi, lo, (name, k))


@pytest.mark.parametrize("k,leaf_cap", [(31, 2048), (21, 2048), (32, 2048), (33, 2048), (63, 2048), (32, 1024), (33, 1024), (63, 1024)])
def test_leaf_merging_edges(kmc, k, leaf_cap):
    """Level-0 children of sizes around the leaf capacity: all exactly leaf_cap, alternating 1 and leaf_cap (+ 1), runs
    that sum to leaf_cap exactly and to one more, occupied digits at the boundaries of the level-0 walk's waves -- with
    leaves of 2048 keys and, for two-word keys, of 1024 (_sort_on_one_ctx)."""
    _sort_on_one_ctx(kmc, k, leaf_cap, ((name, ks.by_digit(k, sizes)) for name, sizes in ks.leaf_edge_sizes(leaf_cap).items()))


# ---- shape 6: leaf sub-bucket skew ----------------------------------------------------------------------------------
SKEW_VARIANTS = ("one_bucket", "equal_33", "equal_most", "equal_2048", "below_bits")


@pytest.mark.parametrize("k,leaf_cap", [(21, 2048), (31, 2048), (33, 2048), (63, 2048), (33, 1024), (63, 1024)])
def test_leaf_sub_bucket_skew(kmc, k, leaf_cap):
    """One leaf whose keys crowd one of its 512 sub-buckets (the second split and the in-wave rank sort): all keys in one
    sub-bucket, 33 equal keys, all but eight keys equal, 2048 equal keys, keys that differ below the sub-bucket bits.
    Leaves of 2048 keys on a fresh ctx (every path); two-word leaves of 1024 keys on a ctx whose sort before collapsed
    its keys (_sort_on_one_ctx) -- one-word keys have leaves of 2048 keys only."""
    cases = [(v, ks.sub_bucket_skew(k, v, leaf_cap)) for v in SKEW_VARIANTS]
    if leaf_cap == 2048:
        for v, (hi, lo) in cases:
            _check_sort(kmc, k, hi, lo, ("skew", k, v))
    else:
        _sort_on_one_ctx(kmc, k, leaf_cap, cases)


# ---- shape 7: the staircase -----------------------------------------------------------------------------------------
def _upload(torch, *arrays):
    out = [torch.from_numpy(a.view(np.int64)).cuda() for a in arrays]
    torch.cuda.synchronize()
    return out


def _merge_pairs(kc, k, d_hi, d_lo, d_w, n):
    kc.merge_pairs_device(d_hi.data_ptr() if k > 31 else 0, d_lo.data_ptr(), d_w.data_ptr(), n)


@pytest.mark.parametrize("k,n_clusters", [(31, 1000), (63, 1000), (63, 32000)])
def test_staircase_unweighted(kmc, k, n_clusters):
    """The staircase (key_shapes.staircase) as reads, core = 2049 keys.  A batch sort's key count is its base positions
    (k per read here), so its lists have k times the room a dense sort has: this is the cross-check of the shape at full
    size (66 M keys of k = 63, fed in pieces: 320,000 terminals in a list of 28.5 M), the tight case is
    test_staircase_weighted."""
    core = 2049
    parts = [ks.staircase(k, min(2000, n_clusters - c), core, first_cluster=c, of_clusters=n_clusters) for c in range(0, n_clusters, 2000)]
    with kmc.KmerCounter(k=k, canonical=False, algo=kmc.ALGO_SORT) as kc:
        for hi, lo in parts:
            _feed(kc, k, hi, lo)
        hi, lo = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        del parts
        want = ks.expected_table(hi, lo)
        assert want[1].shape[0] == n_clusters * (core + 2 * len(ks.staircase_levels(k)))   # all distinct
        t = kc.export()
        assert kc.stats().algo_last == kmc.ALGO_SORT
        assert _eq(t, want) and t.n_total == lo.shape[0]
        del t
        _check_downstream(kc, k, want, seed=n_clusters)


@pytest.mark.parametrize("k,n_clusters", [(31, 1000), (63, 1000), (63, 32000)])
def test_staircase_weighted(kmc, k, n_clusters):
    """The staircase as (key, weight) pairs: kmc_finalize orders the table by ONE weighted sort of n dense keys, whose
    terminal list is the tight one.  Two-word weighted leaves hold 1024 keys, so the core is 1025 (one-word: 2049).

    Terminals per cluster at k = 63: nine shedding levels (2..10) give 18 one-key terminals, the core ends in two leaves:
    20 per cluster of 1043 keys.  The list held 16 * (n / 1024) + 65536 entries, 16.3 per cluster plus 65536 in all --
    short from about 17,700 clusters on: 32,000 clusters (33.4 M keys) make 640,000 terminals against 587,024, and
    kmc_finalize failed with KMC_ERR_CAPACITY, "msd sort: segment / terminal list overflow".  The list is now sized
    from a bound: (2 L + 2) * (n / leaf_cap) + 128 L + 64 with L = ceil(2 k / 10) levels, 28.05 per cluster here (observed
    at 32,000 clusters: 640,000 terminals in a list of 914,332).  At 1,000 clusters the pairs are also merged on top of a
    sorted run of every third key."""
    torch = pytest.importorskip("torch")
    core = 1025 if k > 31 else 2049
    hi, lo = ks.staircase(k, n_clusters, core)
    n = lo.shape[0]
    w = ks.weights_for(n, seed=n_clusters, big=n_clusters == 1000)
    want = ks.expected_table(hi, lo, w)
    assert want[1].shape[0] == n > 131073
    if n_clusters == 1000:
        assert int(w.sum(dtype=np.uint64)) > (1 << 40)
    d_hi, d_lo, d_w = _upload(torch, hi, lo, w)
    with kmc.KmerCounter(k=k, canonical=False) as kc:
        for _ in range(2):
            kc.reset()
            _merge_pairs(kc, k, d_hi, d_lo, d_w, n)
            t = kc.export()
            assert _eq(t, want), (k, n_clusters)
            assert t.n_total == int(w.sum(dtype=np.uint64))
            del t
        _check_downstream(kc, k, want, seed=7)
    if n_clusters == 1000:
        # on top of a sorted run: every third key once more as a read, then the pairs -- the finalize merges table and run
        with kmc.KmerCounter(k=k, canonical=False, algo=kmc.ALGO_SORT) as kc:
            kc.add_batch(*ks.reads_from_keys(hi[::3], lo[::3], k))
            assert kc.export().n_distinct == hi[::3].shape[0] and kc.stats().algo_last == kmc.ALGO_SORT
            _merge_pairs(kc, k, d_hi, d_lo, d_w, n)
            w2 = w.copy(); w2[::3] += np.uint64(1)
            t = kc.export()
            assert _eq(t, ks.expected_table(hi, lo, w2)), (k, "run + table")
            assert t.n_total == int(w.sum(dtype=np.uint64)) + hi[::3].shape[0]


# ---- weighted sorts of the other shapes -----------------------------------------------------------------------------
def _weighted_cases(k):
    leaf = 1024 if k > 31 else 2048   # (weighted leaves: KMC_MSD_LEAF2W / KMC_MSD_LEAF1)
    yield "heavy", ks.heavy_plus_singletons(k, 10, 400_000, "middle")
    yield "prefix_20", ks.shared_prefix(k, 300_000, 20)
    yield "prefix_deep", ks.shared_prefix(k, 300_000, 2 * k - 22)
    for b in (14, 16):   # three (b = 16) or nine (b = 14) spans of all 2^b values under different prefixes
        parts = [ks.low_bits(k, 1 << b, b, True, seed=s) for s in range(3 if b == 16 else 9)]
        for s, (ph, pl) in enumerate(parts):
            pl[:] = (pl[0] & ~np.uint64((1 << b) - 1)) | np.arange(1 << b, dtype=np.uint64)
        yield f"low_{b}", (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
    for name, sizes in ks.leaf_edge_sizes(leaf).items():
        if int(np.sum(sizes)) > 131073:
            yield "digits_" + name, ks.by_digit(k, sizes)


@pytest.mark.parametrize("k", [31, 63])
def test_weighted_sort_of_the_shapes(kmc, k):
    """merge_pairs_device + export on the distinct keys of shapes 2, 3, 4 and 5 (more than 131,073 of them: the weighted
    radix sort, not the small-table finalize), weights up to above 2^32 and, once, a sum above 2^40 (w_total and the run
    totals are 64-bit).  Twice on one ctx with a reset between, and once on top of a sorted run of the same keys, so
    that the finalize merges table and run."""
    torch = pytest.importorskip("torch")
    for i, (name, (hi, lo)) in enumerate(_weighted_cases(k)):
        hi, lo, _ = ks.expected_table(hi, lo)   # the shape's distinct keys
        n = lo.shape[0]
        assert n > 131073, name
        p = np.random.default_rng(i).permutation(n)
        hi, lo = hi[p], lo[p]
        w = ks.weights_for(n, seed=i, big=(i == 0))
        total = int(w.sum(dtype=np.uint64))
        assert (w > (1 << 32)).any() and (i != 0 or total > (1 << 40))
        want = ks.expected_table(hi, lo, w)
        d_hi, d_lo, d_w = _upload(torch, hi, lo, w)
        with kmc.KmerCounter(k=k, canonical=False, algo=kmc.ALGO_SORT) as kc:
            for _ in range(2):
                kc.reset()
                _merge_pairs(kc, k, d_hi, d_lo, d_w, n)
                t = kc.export()
                assert _eq(t, want) and t.n_total == total, (name, k)
            # on top of a sorted run: every third key once more as a read, then the pairs
            kc.reset()
            kc.add_batch(*ks.reads_from_keys(hi[::3], lo[::3], k))
            assert kc.export().n_distinct == hi[::3].shape[0] and kc.stats().algo_last == kmc.ALGO_SORT
            _merge_pairs(kc, k, d_hi, d_lo, d_w, n)
            w2 = w.copy(); w2[::3] += np.uint64(1)
            t = kc.export()
            assert _eq(t, ks.expected_table(hi, lo, w2)) and t.n_total == total + hi[::3].shape[0], (name, k, "run + table")


# ---- shape 8: the count table ---------------------------------------------------------------------------------------
def _table_count(kmc, k, hi, lo, algo, **kw):
    with kmc.KmerCounter(k=k, canonical=False, algo=algo, **kw) as kc:
        _feed(kc, k, hi, lo)
        t = kc.export()
        return t, kc.stats()


@pytest.mark.parametrize("k", [31, 63])
def test_table_shapes(kmc, k):
    """ALGO_STREAM and ALGO_WALK (reads of k bases) on keys that stress probe chains: arithmetic progressions (stride 1,
    2^10, 2^32, the table's capacity), keys that differ in one word only, one key 20 M times (one slot; nothing may
    spill), 3 M distinct keys into a ctx created with capacity_hint = 1 (growth and spill)."""
    algos = (kmc.ALGO_STREAM, kmc.ALGO_WALK)
    with kmc.KmerCounter(k=k, canonical=False, algo=kmc.ALGO_STREAM) as kc:
        kc.add_batch(*ks.reads_from_keys(*ks.one_key(k, 4), k))
        kc.finalize()
        cap = int(kc.stats().table_capacity)
    assert cap >= 1024 and cap & (cap - 1) == 0
    cases = [(f"stride_{s}", ks.arithmetic(k, 300_000, s, start=12345)) for s in (1, 1 << 10, 1 << 32, cap)]
    if k > 32:
        cases += [("high_word", ks.one_word_differs(k, 300_000, "high")), ("low_word", ks.one_word_differs(k, 300_000, "low"))]
    for name, (hi, lo) in cases:
        want = ks.expected_table(hi, lo)
        for algo in algos:
            t, st = _table_count(kmc, k, hi, lo, algo)
            assert _eq(t, want) and t.n_total == lo.shape[0], (name, k, algo)
    hi, lo = ks.one_key(k, 20_000_000)
    want = ks.expected_table(hi, lo)
    for algo in algos:
        t, st = _table_count(kmc, k, hi, lo, algo)
        assert _eq(t, want) and t.n_total == 20_000_000, (k, algo)
        assert st.n_spilled == 0, (k, algo)
    hi, lo = ks.random_bits(np.random.default_rng(k), 3_000_000, 2 * k)
    want = ks.expected_table(hi, lo)
    for algo in algos:
        t, st = _table_count(kmc, k, hi, lo, algo, capacity_hint=1)
        assert _eq(t, want) and t.n_total == 3_000_000, (k, algo)


# ---- the canonical strand -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 31, 32, 63])
def test_canonical_strand(kmc, k):
    """Shapes 1, 2 and 3 with canonical=True: the expected keys are min(key, revcomp(key)), computed in numpy."""
    for what, (hi, lo) in (("one_key", ks.one_key(k, 70_000)),
                           ("heavy", ks.heavy_plus_singletons(k, 400_000, 100_000, "smallest")),
                           ("zipf", ks.zipf_heavy(k, 200_000, 100_000)),
                           ("prefix_20", ks.shared_prefix(k, 300_000, 20)),
                           ("prefix_deep", ks.shared_prefix(k, 300_000, 2 * k - 12))):
        _check_sort(kmc, k, hi, lo, (what, k, "canonical"), canonical=True)


# ---- LR mode --------------------------------------------------------------------------------------------------------
def test_lr_mode_rank_shapes(kmc, oracle):
    """The reference's 27 + gap + 27 mode on reads of 80 bases (one chunk each): one 27-mer rank, two ranks, one heavy
    pair among distinct ones, and halves that differ in their low bits only -- against the oracle, and against the
    numpy table of the 54-mer keys."""
    rng = np.random.default_rng(21)
    n = 40_000
    _, L = ks.random_bits(rng, n, 54)
    _, R = ks.random_bits(rng, n, 54)
    cases = {"distinct": (L, R)}
    cases["one_rank"] = (np.full(n, L[0]), np.full(n, L[0]))
    cases["two_ranks"] = (L[rng.integers(0, 2, n)], L[rng.integers(0, 2, n)])
    l, r = L.copy(), R.copy(); l[: n - 5000] = L[0]; r[: n - 5000] = R[0]
    cases["heavy_pair"] = (l, r)
    for b in (1, 6, 14):
        _, x = ks.low_bits(27, n, b, True, seed=b)
        _, y = ks.low_bits(27, n, b, False, seed=b + 50)
        cases[f"low_{b}"] = (x, y)
    for name, (l, r) in cases.items():
        bases, offs = ks.lr_reads_from_halves(l, r)
        want = oracle.count_lr(bases, offs)
        assert _eq(want, ks.expected_table(*ks.lr_keys(l, r))), name
        with kmc.KmerCounter(mode=kmc.MODE_LR) as kc:
            kc.add_batch(bases, offs)
            t = kc.export()
            assert t.equals(want) and t.n_total == n, name
