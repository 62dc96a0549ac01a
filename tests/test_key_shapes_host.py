"""The key-injection helper (tests/key_shapes.py) against the C oracle, on the CPU: for every shape the reads that
reads_from_keys() builds give, counted by the oracle, exactly the table expected_table() computes from the keys with
numpy -- so the GPU tests (test_key_shapes_gpu.py) may use expected_table() at sizes the oracle would take minutes for."""
import importlib

import numpy as np
import pytest

import key_shapes as ks

KS = (5, 31, 32, 63)


def _same(t, exp):
    eh, el, ec = exp
    return np.array_equal(t.key_hi, eh) and np.array_equal(t.key_lo, el) and np.array_equal(t.count, ec)


def _shapes(k):
    """(name, hi, lo) of every shape at a few thousand keys, where k has room for it."""
    kb = 2 * k
    yield "one_key", *ks.one_key(k, 3000)
    for where in ("smallest", "largest", "middle"):
        yield "heavy_" + where, *ks.heavy_plus_singletons(k, 3000, 1000, where)
    yield "zipf", *ks.zipf_heavy(k, 1000, 1000)
    for p in (9, 10, 11, 20, 40, 61, 64, 100, 120):
        if p < kb - 1:
            yield f"prefix_{p}", *ks.shared_prefix(k, 3000, p)
    for b in (1, 6, 13, 14, 15, 16):
        if b < kb:
            yield f"low_{b}_dense", *ks.low_bits(k, 3000, b, True)
            yield f"low_{b}_sparse", *ks.low_bits(k, 3000, b, False)
    if kb >= 30:
        for name, sizes in ks.leaf_edge_sizes(8).items():
            yield "digits_" + name, *ks.by_digit(k, sizes)
        for v in ("one_bucket", "equal_33", "equal_most", "equal_2048", "below_bits"):
            yield "leaf_" + v, *ks.sub_bucket_skew(k, v)
    if kb >= 42:
        yield "staircase", *ks.staircase(k, 6, 1025)
    for stride in (1, 1 << 10, 1 << 32, 1 << 21):
        yield f"arith_{stride}", *ks.arithmetic(k, 3000, stride, 7)
    if k >= 33:
        yield "high_word", *ks.one_word_differs(k, 3000, "high")
        yield "low_word", *ks.one_word_differs(k, 3000, "low")


@pytest.mark.parametrize("k", KS)
def test_every_shape_matches_the_oracle(oracle, k):
    mh, ml = ks.key_mask(k)
    seen = set()
    for name, hi, lo in _shapes(k):
        assert hi.dtype == np.uint64 and lo.dtype == np.uint64 and hi.shape == lo.shape, name
        assert not (hi & ~np.uint64(mh)).any() and not (lo & ~np.uint64(ml)).any(), name   # keys stay below 4^k
        bases, offs = ks.reads_from_keys(hi, lo, k)
        assert bases.shape[0] == k * lo.shape[0] and offs[-1] == bases.shape[0]
        want = ks.expected_table(hi, lo)
        assert int(want[2].sum()) == lo.shape[0], name
        assert _same(oracle.count_kmers(bases, offs, k, False), want), (name, k)
        seen.add(name.split('_')[0])
    want_kinds = {'one', 'heavy', 'zipf', 'low', 'arith'} | (set() if k == 5 else {'prefix', 'digits', 'leaf', 'staircase'})
    assert want_kinds <= seen   # (k = 5 has room for the short shapes only)


@pytest.mark.parametrize("k", KS)
def test_generators_are_deterministic_and_weights_sum(k):
    a = ks.zipf_heavy(k, 500, 500)
    b = ks.zipf_heavy(k, 500, 500)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    w = ks.weights_for(a[1].shape[0], big=True)
    assert (w > (1 << 32)).any() and int(w.sum(dtype=np.uint64)) > (1 << 40)
    eh, el, ec = ks.expected_table(a[0], a[1], w)
    assert int(ec.sum(dtype=np.uint64)) == int(w.sum(dtype=np.uint64))
    # the weighted table against a dictionary
    d = {}
    for key, wi in zip(ks.to_ints(*a), w.tolist()):
        d[key] = d.get(key, 0) + wi
    assert ks.to_ints(eh, el) == sorted(d) and ec.tolist() == [d[x] for x in sorted(d)]


@pytest.mark.parametrize("k", KS)
def test_decoded_reads_round_trip_through_encode_key(k):
    kmc = importlib.import_module("k-mer-count_amd")
    try:
        kmc.lib()
    except Exception as e:   # the library is built by build(); without it there is nothing to round-trip through
        pytest.fail(f"libkmc.so is not built: {e}")
    hi, lo = ks.zipf_heavy(k, 20, 60)
    rows = ks.decode_keys(hi, lo, k)
    assert rows.shape == (lo.shape[0], k)
    for i in range(rows.shape[0]):
        assert kmc.encode_key(rows[i].tobytes().decode(), canonical=False) == (int(hi[i]), int(lo[i])), (k, i)


@pytest.mark.parametrize("k", KS)
def test_canonical_keys_match_the_oracle(oracle, k):
    for hi, lo in (ks.one_key(k, 100), ks.zipf_heavy(k, 300, 2000), ks.shared_prefix(k, 2000, min(9, 2 * k - 2))):
        bases, offs = ks.reads_from_keys(hi, lo, k)
        ch, cl = ks.canonical_keys(hi, lo, k)
        assert _same(oracle.count_kmers(bases, offs, k, True), ks.expected_table(ch, cl)), k
        # an involution, and the palindrome-free check: revcomp twice is the key
        rh, rl = ks.revcomp(*ks.revcomp(hi, lo, k), k)
        assert np.array_equal(rh, hi) and np.array_equal(rl, lo)


def test_lr_reads_match_the_oracle(oracle):
    rng = np.random.default_rng(12)
    _, L = ks.random_bits(rng, 3000, 54)
    _, R = ks.random_bits(rng, 3000, 54)
    for name in ("one_rank", "two_ranks", "distinct"):
        l, r = L.copy(), R.copy()
        if name == "one_rank":
            l[:] = L[0]; r[:] = L[0]
        elif name == "two_ranks":
            l[:] = L[rng.integers(0, 2, 3000)]; r[:] = L[rng.integers(0, 2, 3000)]
        bases, offs = ks.lr_reads_from_halves(l, r)
        assert bases.shape[0] == 80 * 3000
        t = oracle.count_lr(bases, offs)
        assert t.klen == 54 and _same(t, ks.expected_table(*ks.lr_keys(l, r))), name


def test_staircase_structure():
    """What the staircase promises, checked on the keys themselves: per cluster and shedding level exactly one key below
    and one above the core's digit, the core in digit 512, and cores that differ in their low twelve bits only."""
    k, C, core = 63, 5, 1025
    kb = 2 * k
    levels = ks.staircase_levels(k)
    assert levels == list(range(2, 11))
    hi, lo = ks.staircase(k, C, core)
    keys = np.array(ks.to_ints(hi, lo), dtype=object)
    assert len(set(keys.tolist())) == C * (core + 2 * len(levels))
    cid = keys >> (kb - 20)
    for c in sorted(set(cid.tolist())):
        mine = keys[cid == c]
        alive = mine
        for j in levels:
            d = (alive >> (kb - 10 * (j + 1))) & 1023
            assert int((d < 512).sum()) == 1 and int((d > 512).sum()) == 1, (c, j)
            alive = alive[d == 512]
        assert alive.shape[0] == core and len(set((alive >> 12).tolist())) == 1
    # fed in pieces, the clusters are the same keys as in one call with the same numbering
    a = ks.staircase(k, 2, core, first_cluster=2, of_clusters=8)
    b = ks.staircase(k, 2, core, first_cluster=2, of_clusters=8)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert set((np.array(ks.to_ints(*a), dtype=object) >> (kb - 20)).tolist()) == {2 << 17, 3 << 17}
