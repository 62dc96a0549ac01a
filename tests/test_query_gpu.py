"""GPU checks of kmc_query / kmc_query_device / kmc_profile / kmc_profile_device (kmc_query.hip.h).  Expected values share
no code with the kernels: the CPU oracle's table turned into a Python dict, and a plain-Python window walker (slice,
reverse complement by string, min, dict lookup).  All comparisons are exact."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SAMPLE

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "bin", "k-mer-count")
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
U64 = np.uint64


def _rc(s: bytes) -> bytes:
    return s[::-1].translate(_COMP)


def _table_dict(t):
    """{k-mer bytes: count} of an oracle table."""
    km = t.kmers()
    return {km[i].tobytes(): int(t.count[i]) for i in range(t.n_distinct)}


def _walk(bases, offs, k, canonical, table, min_count=1):
    """The model: per window start the count (python ints), per read [valid, present, min, max, sum]."""
    raw = bytes(np.asarray(bases, np.uint8))
    win = [0] * len(raw)
    stats = []
    thr = max(int(min_count), 1)
    for r in range(len(offs) - 1):
        a, b = int(offs[r]), int(offs[r + 1])
        s = raw[a:b]
        cs = []
        for j in range(len(s) - k + 1):
            w = s[j:j + k]
            if w.translate(None, b"ACGT"):   # something is left when the ACGT bytes are deleted
                continue
            key = min(w, _rc(w)) if canonical else w
            c = table.get(key, 0)
            win[a + j] = c
            cs.append(c)
        stats.append([len(cs), sum(1 for c in cs if c >= thr), min(cs) if cs else 0, max(cs) if cs else 0, sum(cs)])
    return win, np.array(stats, dtype=U64).reshape(len(offs) - 1, 5)


def _sat32(win):
    return np.array([min(c, 0xFFFFFFFF) for c in win], dtype=np.uint32)


def _dev(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a, dtype=U64).view(np.int64), device="cuda")


def _query_device(kc, hi, lo, use_hi):
    import torch
    n = len(lo)
    d_lo, d_hi = _dev(lo), _dev(hi)
    out = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    kc.query_device(d_hi.data_ptr() if use_hi else 0, d_lo.data_ptr(), n, out.data_ptr())
    kc.sync()
    return out.cpu().numpy().view(U64).copy()


def _absent_keys(t, kbits, full=None):
    """each key of t +- 1 where that is not a key of the table, 0 and the all-ones key of kbits bits (unless present)"""
    full = full or t
    have = set(zip(full.key_hi.tolist(), full.key_lo.tolist()))
    top = (1 << kbits) - 1
    cand = {0, top}
    for h, l in zip(t.key_hi.tolist(), t.key_lo.tolist()):
        v = (h << 64) | l
        cand.add(v + 1 if v < top else v)
        cand.add(v - 1 if v else 0)
    cand = sorted(v for v in cand if ((v >> 64), v & (2**64 - 1)) not in have)
    return np.array([v >> 64 for v in cand], U64), np.array([v & (2**64 - 1) for v in cand], U64)


def _check_lookups(kc, t, kbits, rng, full=None):
    two = kbits > 64
    got = kc.query(t.key_lo, t.key_hi)
    assert np.array_equal(got, t.count)
    if not two:
        assert np.array_equal(kc.query(t.key_lo), t.count)            # key_hi omitted
    ahi, alo = _absent_keys(t, kbits, full)
    assert len(alo) or kbits == 2
    assert not kc.query(alo, ahi).any()
    # shuffled, with duplicates, present and absent mixed
    n = t.n_distinct
    if n:
        pick = rng.integers(0, n, 2 * n + 7)
        qhi = np.concatenate([t.key_hi[pick], ahi])
        qlo = np.concatenate([t.key_lo[pick], alo])
        want = np.concatenate([t.count[pick], np.zeros(len(alo), U64)])
        p = rng.permutation(len(qlo))
        qhi, qlo, want = qhi[p], qlo[p], want[p]
        assert np.array_equal(kc.query(qlo, qhi), want)
        assert np.array_equal(_query_device(kc, qhi, qlo, True), want)
        if not two:
            assert np.array_equal(_query_device(kc, qhi, qlo, False), want)
        # an odd start (8-byte but not 16-byte aligned device arrays)
        import torch
        d_lo, d_hi = _dev(np.concatenate([np.zeros(1, U64), qlo])), _dev(np.concatenate([np.zeros(1, U64), qhi]))
        out = torch.full((len(qlo) + 1,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        kc.query_device(d_hi.data_ptr() + 8, d_lo.data_ptr() + 8, len(qlo), out.data_ptr() + 8)
        kc.sync()
        o = out.cpu().numpy().view(U64)
        assert np.array_equal(o[1:], want) and o[0] == U64(2**64 - 1)
    assert kc.query(np.zeros(0, U64)).shape == (0,)
    kc.query_device(0, 0, 0, 0)


@pytest.mark.parametrize("k", [5, 21, 31, 63])
def test_lookups_sample_fasta_every_algo(kmc, oracle, k):
    bases, offs = kmc.parse_fasta(SAMPLE)
    rng = np.random.default_rng(k)
    for canonical in (True, False):
        want = oracle.count_kmers(bases, offs, k, canonical)
        for algo in (kmc.ALGO_STREAM, kmc.ALGO_WALK, kmc.ALGO_SORT, kmc.ALGO_AUTO):
            with kmc.KmerCounter(k=k, canonical=canonical, algo=algo) as kc:
                kc.add_batch(bases, offs)
                kc.finalize()
                _check_lookups(kc, want, 2 * k, rng)
                if algo == kmc.ALGO_AUTO:
                    km = want.kmers()
                    sel = rng.integers(0, want.n_distinct, 200)
                    strs = [km[i].tobytes().decode() for i in sel]
                    assert np.array_equal(kc.query_kmers(strs), want.count[sel])
                    if canonical:   # the other strand of a canonical k-mer is the same k-mer
                        assert np.array_equal(kc.query_kmers([_rc(s.encode()) for s in strs]), want.count[sel])


def test_lookups_reference_mode(kmc, oracle):
    bases, offs = kmc.parse_fasta(SAMPLE)
    want = oracle.count_lr(bases, offs)
    rng = np.random.default_rng(54)
    with kmc.KmerCounter(mode=kmc.MODE_LR) as kc:
        kc.count_file(SAMPLE)
        kc.finalize()
        sub = rng.choice(want.n_distinct, 50000, replace=False)
        sub.sort()
        Table = type(want)
        _check_lookups(kc, Table(want.key_hi[sub], want.key_lo[sub], want.count[sub], want.klen), 108, rng, want)
        assert np.array_equal(kc.query(want.key_lo, want.key_hi), want.count)
        with pytest.raises(kmc.KmcError) as e:
            kc.profile(bases[:100], np.array([0, 100], U64))
        assert e.value.status == kmc.ERR_ARG


def _random_reads(rng, n_reads, lo, hi):
    lens = rng.integers(lo, hi + 1, n_reads)
    offs = np.zeros(n_reads + 1, U64)
    offs[1:] = np.cumsum(lens)
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(offs[-1]))]
    return bases, offs


def _check_view(kc, rng, kbits, want=None):
    L = kc._L
    nd, _ = kc.finalize()
    hi, lo, cnt = np.zeros(nd, U64), np.zeros(nd, U64), np.zeros(nd, U64)
    kc._chk(L.kmc_export(kc._h, hi.ctypes.data, lo.ctypes.data, cnt.ctypes.data, nd))
    import importlib as il
    T = il.import_module("k-mer-count_amd").Table
    t = T(hi, lo, cnt, kc.k)
    if want is not None:
        assert t.equals(want)
    full = t
    if nd > 200000:   # keep the +-1 neighbour sets of big views small
        sub = np.sort(rng.choice(nd, 100000, replace=False))
        assert np.array_equal(kc.query(lo, hi), cnt)
        t = T(hi[sub], lo[sub], cnt[sub], kc.k)
    _check_lookups(kc, t, kbits, rng, full)


def test_every_way_a_view_comes_to_be(kmc, oracle, monkeypatch):
    rng = np.random.default_rng(11)
    hb, ho = kmc.synth_reads_host(kmc.Synth(seed=4), 0, 3000)
    want = oracle.count_kmers(hb, ho, 31, True)
    # small-table kernel
    with kmc.KmerCounter(k=31) as kc:
        kc.add_batch(hb, ho)
        _check_view(kc, rng, 62, want)
    # a view queued by finalize_async and never observed before the query
    for form in ("query", "query_device", "profile"):
        with kmc.KmerCounter(k=31) as kc:
            kc.add_batch(hb, ho)
            kc.export()
            kc.reset()
            kc.add_batch(hb, ho)
            ok0 = kc.stats().n_async_ok
            kc.finalize_async()
            if form == "query":
                assert np.array_equal(kc.query(want.key_lo), want.count)
            elif form == "query_device":
                assert np.array_equal(_query_device(kc, want.key_hi, want.key_lo, False), want.count)
            else:
                win, rs = kc.profile(hb[:int(ho[20])], ho[:21])
                mw, ms = _walk(hb[:int(ho[20])], ho[:21], 31, True, _table_dict(want))
                assert np.array_equal(win, _sat32(mw)) and np.array_equal(rs, ms)
            assert kc.finalize() == (want.n_distinct, want.n_total)
            assert kc.stats().n_async_ok == ok0 + 1
    # both sides of the small-table kernel's 131072-key limit
    monkeypatch.setenv("KMC_FIN_SMALL_MAX", "131072")
    for n in (131072, 131073):
        lo = np.unique(rng.integers(0, 1 << 62, 2 * n, dtype=U64))[:n]
        cnt = rng.integers(1, 9, n).astype(U64)
        p = rng.permutation(n)
        with kmc.KmerCounter(k=31) as kc:
            d_lo, d_cnt = _dev(lo[p]), _dev(cnt[p])
            kc.merge_pairs_device(0, d_lo.data_ptr(), d_cnt.data_ptr(), n)
            T = kmc.Table
            _check_view(kc, rng, 62, T(np.zeros(n, U64), lo, cnt, 31))
    monkeypatch.delenv("KMC_FIN_SMALL_MAX")
    # sort path: one run, then several runs (all-distinct synthetic reads, pool 0), then table + runs merged
    for k in (31, 63):
        sb, so = kmc.synth_reads_host(kmc.Synth(seed=9, pool=0), 0, 6000)
        with kmc.KmerCounter(k=k, algo=kmc.ALGO_SORT) as kc:
            kc.add_batch(sb, so)
            _check_view(kc, rng, 2 * k, oracle.count_kmers(sb, so, k, True, method=1))
            for first in (6000, 12000):
                b2, o2 = kmc.synth_reads_host(kmc.Synth(seed=9, pool=0), first, 6000)
                kc.add_batch(b2, o2)
                kc.finalize()
            ab, ao = kmc.synth_reads_host(kmc.Synth(seed=9, pool=0), 0, 18000)
            _check_view(kc, rng, 2 * k, oracle.count_kmers(ab, ao, k, True, method=1))
    bases, offs = _random_reads(rng, 20000, 300, 400)
    with kmc.KmerCounter(k=31) as kc:
        kc.add_batch(bases, offs)
        kc.add_batch(bases[:int(offs[5000])], offs[:5001])
        _check_view(kc, rng, 62)
    # an empty view: zeros
    with kmc.KmerCounter(k=31) as kc:
        kc.finalize()
        assert not kc.query(np.array([0, 5, 2**62 - 1], U64)).any()
        win, rs = kc.profile(hb[:int(ho[3])], ho[:4])
        assert not win.any() and np.array_equal(rs[:, 0], np.full(3, 400 - 30, U64)) and not rs[:, 1:].any()


def _merged(kmc, k, hi, lo, cnt):
    kc = kmc.KmerCounter(k=k)
    d_hi, d_lo, d_cnt = _dev(hi), _dev(lo), _dev(cnt)
    kc.merge_pairs_device(d_hi.data_ptr() if k > 31 else 0, d_lo.data_ptr(), d_cnt.data_ptr(), len(lo))
    assert kc.finalize()[0] == len(lo)
    return kc


def test_adversarial_shapes(kmc):
    rng = np.random.default_rng(5)
    T = kmc.Table
    shapes = []
    for n in (1, 2, 3):
        shapes.append((31, np.zeros(n, U64), np.sort(rng.integers(1, 1 << 62, n, dtype=U64))))
    # thousands of keys that share all but their low 12 bits: one bucket holds everything
    base = U64(0x2AAAAAAAAAAAA000)
    shapes.append((31, np.zeros(4096, U64), base + np.arange(4096, dtype=U64)))
    shapes.append((31, np.zeros(3000, U64), base + np.sort(rng.choice(4096, 3000, replace=False)).astype(U64)))
    # keys only in the first and the last bucket
    ends = np.concatenate([np.arange(0, 700, dtype=U64), U64(2**62 - 1) - np.arange(0, 700, dtype=U64)[::-1]])
    shapes.append((31, np.zeros(len(ends), U64), ends))
    # key 0 and the largest key alone
    shapes.append((31, np.zeros(2, U64), np.array([0, 2**62 - 1], U64)))
    shapes.append((5, np.zeros(2, U64), np.array([0, 2**10 - 1], U64)))
    shapes.append((1, np.zeros(4, U64), np.arange(4, dtype=U64)))
    # two-word keys: equal in hi and differing in lo, and the reverse
    lo2 = np.sort(rng.integers(0, 1 << 63, 5000, dtype=U64) * U64(2) + U64(1))
    lo2 = np.unique(lo2)
    shapes.append((63, np.full(len(lo2), 12345, U64), lo2))
    hi2 = np.unique(rng.integers(0, 1 << 62, 5000, dtype=U64))
    shapes.append((63, hi2, np.full(len(hi2), 0xDEADBEEF, U64)))
    shapes.append((63, np.array([0, 2**62 - 1], U64), np.array([0, 2**64 - 1], U64)))
    shapes.append((32, np.zeros(3, U64), np.array([0, 7, 2**64 - 1], U64)))
    for k, hi, lo in shapes:
        n = len(lo)
        cnt = rng.integers(1, 1000, n).astype(U64)
        p = rng.permutation(n)
        kc = _merged(kmc, k, hi[p], lo[p], cnt[p])
        try:
            _check_view(kc, rng, 2 * k, T(hi, lo, cnt, k))
            # keys beyond the ctx's key bits are absent, not an error
            assert not kc.query(np.array([2**64 - 1, 0], U64), np.array([2**64 - 1, 2**63], U64)).any()
        finally:
            kc.close()


def test_millions_of_keys_random_queries(kmc, oracle):
    rng = np.random.default_rng(17)
    sb, so = kmc.synth_reads_host(kmc.Synth(seed=21, pool=0), 0, 12000)   # 12000 x 400 bases: ~4.4 M distinct 31-mers
    want = oracle.count_kmers(sb, so, 31, True, method=1)
    assert want.n_distinct > 4_000_000
    with kmc.KmerCounter(k=31) as kc:
        kc.add_batch(sb, so)
        kc.finalize()
        nq = 1_000_000
        pick = rng.integers(0, want.n_distinct, nq // 2)
        rnd = rng.integers(0, 1 << 62, nq - nq // 2, dtype=U64)
        q = np.concatenate([want.key_lo[pick], rnd])
        pos = np.searchsorted(want.key_lo, rnd)
        hit = (pos < want.n_distinct) & (want.key_lo[np.minimum(pos, want.n_distinct - 1)] == rnd)
        exp = np.concatenate([want.count[pick], np.where(hit, want.count[np.minimum(pos, want.n_distinct - 1)], 0).astype(U64)])
        p = rng.permutation(nq)
        assert np.array_equal(kc.query(q[p]), exp[p])
        assert np.array_equal(_query_device(kc, np.zeros(nq, U64), q[p], False), exp[p])


def test_cache_invalidation_and_state_errors(kmc, oracle):
    L = kmc.lib()
    bases, offs = kmc.parse_fasta(SAMPLE)
    want = oracle.count_kmers(bases, offs, 31, True)
    half = len(offs) // 2
    b1, o1 = bases[:int(offs[half])], offs[:half + 1]
    w1 = oracle.count_kmers(b1, o1, 31, True)

    def states_equal(kc):
        """every new call answers what kmc_export answers in this state"""
        one = np.zeros(1, U64)
        rc = L.kmc_export(kc._h, None, None, None, 0)
        rc = kmc.ERR_STATE if rc == kmc.ERR_STATE else kmc.OK   # (a valid view: export complains about the capacity instead)
        out = np.zeros(1, U64)
        assert (L.kmc_query(kc._h, None, one.ctypes.data, 1, out.ctypes.data) == kmc.ERR_STATE) == (rc == kmc.ERR_STATE)
        assert (L.kmc_query_device(kc._h, None, None, 0, None) == kmc.ERR_STATE) == (rc == kmc.ERR_STATE)
        assert (L.kmc_profile(kc._h, None, None, 0, 1, None, None) == kmc.ERR_STATE) == (rc == kmc.ERR_STATE)
        assert (L.kmc_profile_device(kc._h, None, None, 0, 0, 1, None, None) == kmc.ERR_STATE) == (rc == kmc.ERR_STATE)
        return rc

    with kmc.KmerCounter(k=31) as kc:
        assert states_equal(kc) == kmc.ERR_STATE          # before any finalize
        kc.add_batch(b1, o1)
        assert states_equal(kc) == kmc.ERR_STATE
        kc.finalize()
        assert states_equal(kc) == kmc.OK
        assert np.array_equal(kc.query(w1.key_lo), w1.count)
        got = kc.query(want.key_lo)
        d1 = dict(zip(w1.key_lo.tolist(), w1.count.tolist()))
        assert got.tolist() == [d1.get(x, 0) for x in want.key_lo.tolist()]
        kc.add_batch(bases[int(offs[half]):], offs[half:] - offs[half])
        assert states_equal(kc) == kmc.ERR_STATE          # the view is stale
        kc.finalize()
        assert np.array_equal(kc.query(want.key_lo), want.count)    # new counts, not the cached index's
        kc.reset()
        assert states_equal(kc) == kmc.ERR_STATE
        kc.finalize()
        assert not kc.query(want.key_lo).any()
        kc.add_batch(b1, o1)
        kc.finalize()
        assert np.array_equal(kc.query(w1.key_lo), w1.count)


def _profile_batch(rng, k):
    """(counted reads, profiled reads): the profiled ones are the counted ones with a share of bases mutated."""
    lens = [0, 1, max(k - 1, 0), k, k + 1, 0, 5000, 70000, 37, 0] + [150] * 2500 + [k, 0]
    offs = np.zeros(len(lens) + 1, U64)
    offs[1:] = np.cumsum(lens)
    counted = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(offs[-1]))].copy()
    counted[int(offs[6]):int(offs[6]) + 2000] = counted[int(offs[7]):int(offs[7]) + 2000]   # repeats: counts above 1
    counted[int(offs[10]):int(offs[700])] = counted[int(offs[700]):int(offs[700]) + int(offs[700]) - int(offs[10])]
    prof = counted.copy()
    mut = rng.random(len(prof)) < 0.01
    prof[mut] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(mut.sum()))]
    odd = rng.random(len(prof)) < 0.002
    prof[odd] = np.frombuffer(b"NacgtRn-", np.uint8)[rng.integers(0, 8, int(odd.sum()))]
    return counted, prof, offs


@pytest.mark.parametrize("k", [1, 5, 31, 32, 33, 63])
def test_profiles_against_the_walker(kmc, oracle, k):
    import torch
    rng = np.random.default_rng(100 + k)
    counted, prof, offs = _profile_batch(rng, k)
    for canonical in (True, False):
        want = oracle.count_kmers(counted, offs, k, canonical)
        table = _table_dict(want)
        top = int(want.count.max())
        with kmc.KmerCounter(k=k, canonical=canonical) as kc:
            kc.add_batch(counted, offs)
            kc.finalize()
            digest = kc.export().digest()
            for min_count in (1, 2, top + 1):
                mw, ms = _walk(prof, offs, k, canonical, table, min_count)
                win, rs = kc.profile(prof, offs, min_count)
                bad = np.nonzero(win != _sat32(mw))[0]
                assert not len(bad), (k, canonical, bad[:10], win[bad[:10]], [mw[i] for i in bad[:10]])
                badr = np.nonzero((rs != ms).any(axis=1))[0]
                assert not len(badr), (k, canonical, min_count, badr[:5], rs[badr[:5]], ms[badr[:5]])
                if k >= 31:
                    assert all(any(c == 0 for c in mw[int(offs[r]):int(offs[r + 1]) - k + 1]) for r in (6, 7))
            # either output alone
            w_only, none = kc.profile(prof, offs, 1, stats=False)
            assert none is None and np.array_equal(w_only, win)
            none, s_only = kc.profile(prof, offs, top + 1, windows=False)
            assert none is None and np.array_equal(s_only, rs)
            # device form (padded to 16 bytes as kmc_add_batch_device asks)
            pad = np.zeros((len(prof) + 15) // 16 * 16, np.uint8)
            pad[:len(prof)] = prof
            d_b = torch.tensor(pad, device="cuda")[:len(prof)]
            d_o = torch.tensor(offs.view(np.int64), device="cuda")
            dw, ds = kc.profile_tensors(d_b, d_o, top + 1)
            kc.sync()
            assert np.array_equal(dw.cpu().numpy().view(np.uint32), win) and np.array_equal(ds.cpu().numpy().view(U64), rs)
            dw, none = kc.profile_tensors(d_b, d_o, 1, stats=False)
            kc.sync()
            assert none is None and np.array_equal(dw.cpu().numpy().view(np.uint32), win)
            assert kc.export().digest() == digest


def test_profile_saturation(kmc):
    k = 31
    rng = np.random.default_rng(3)
    read = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 100)]
    L = kmc.lib()
    keys = [kmc.encode_key(bytes(read[j:j + k]), True) for j in range(100 - k + 1)]
    big = (1 << 32) + 5
    lo = np.array([keys[10][1], keys[40][1]], U64)
    cnt = np.array([big, 7], U64)
    kc = _merged(kmc, k, np.zeros(2, U64), lo, cnt)
    try:
        win, rs = kc.profile(read, np.array([0, 100], U64))
        assert win[10] == 0xFFFFFFFF and win[40] == 7 and int(win.astype(U64).sum()) == 0xFFFFFFFF + 7
        assert rs.tolist() == [[70, 2, 0, big, big + 7]]
        assert kc.query(lo).tolist() == [big, 7]
    finally:
        kc.close()


def _dev_u64(ptr, n):
    kd = importlib.import_module("k-mer-count_amd.distributed")
    import torch
    return kd.device_view(ptr, n, torch.device("cuda", 0)).cpu().numpy().view(U64).copy()


def test_nothing_is_disturbed(kmc, oracle):
    bases, offs = kmc.parse_fasta(SAMPLE)
    for k in (31, 63):
        want = oracle.count_kmers(bases, offs, k, True)
        with kmc.KmerCounter(k=k) as kc:
            kc.add_batch(bases, offs)
            kc.finalize()
            digest = kc.export().digest()
            vp = kc.export_device()
            fhi, flo, fcnt, nk, _ = kc.filter_device(2, 0)
            pb, phi, plo, pcnt = kc.partition_device(4)
            n = pb[-1]
            before = [_dev_u64(p, m) for p, m in ((plo, n), (pcnt, n), (flo, nk), (fcnt, nk))]
            assert np.array_equal(kc.query(want.key_lo, want.key_hi), want.count)
            sub = int(offs[min(40, len(offs) - 1)])
            kc.profile(bases[:sub], offs[:min(40, len(offs) - 1) + 1])
            after = [_dev_u64(p, m) for p, m in ((plo, n), (pcnt, n), (flo, nk), (fcnt, nk))]
            assert all(np.array_equal(a, b) for a, b in zip(before, after))
            assert kc.export_device() == vp and kc.export().digest() == digest
            kc.add_batch(bases, offs)
            t = kc.export()
            assert np.array_equal(t.key_lo, want.key_lo) and np.array_equal(t.count, want.count * U64(2))
            assert np.array_equal(kc.query(want.key_lo, want.key_hi), want.count * U64(2))


@pytest.mark.parametrize("forward", [False, True])
def test_cli_query_and_profile(kmc, oracle, tmp_path, forward):
    k = 21
    bases, offs = kmc.parse_fasta(SAMPLE)
    want = oracle.count_kmers(bases, offs, k, not forward)
    table = _table_dict(want)
    rng = np.random.default_rng(8)
    km = want.kmers()
    kmers = [km[i].tobytes() for i in rng.integers(0, want.n_distinct, 50)]
    kmers += [_rc(x) for x in kmers[:20]] + [bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, k)]) for _ in range(20)]
    qf = tmp_path / "q.txt"
    qf.write_bytes(b"".join(x + b"\n" for x in kmers))
    model = b"".join(x + b"\t%d\n" % table.get(x if forward else min(x, _rc(x)), 0) for x in kmers)
    fw = ["--forward"] if forward else []
    r = subprocess.run([EXE, SAMPLE, "-k", str(k), "--query-kmers", str(qf)] + fw, capture_output=True)
    assert r.returncode == 0 and r.stdout == model, r.stderr
    # profile: a few reads of the sample, some bases changed, as FASTA
    raw = bytes(bases)
    reads = []
    for r_i in range(min(12, len(offs) - 1)):
        s = bytearray(raw[int(offs[r_i]):int(offs[r_i + 1])][:600])
        for j in range(7, len(s), 53):
            s[j] = b"ACGT"[(b"ACGT".index(s[j]) + 1) % 4] if s[j] in b"ACGT" else s[j]
        reads.append(bytes(s))
    pf = tmp_path / "p.fasta"
    pf.write_bytes(b"".join(b">r%d\n" % i + s + b"\n" for i, s in enumerate(reads)))
    po = np.zeros(len(reads) + 1, U64)
    po[1:] = np.cumsum([len(s) for s in reads])
    for mc in (1, 3):
        _, ms = _walk(np.frombuffer(b"".join(reads), np.uint8), po, k, not forward, table, mc)
        model = b"".join(b"%d\t%d\t%d\t%d\t%d\t%d\n" % ((i,) + tuple(int(x) for x in ms[i])) for i in range(len(reads)))
        r = subprocess.run([EXE, SAMPLE, "-k", str(k), "--profile", str(pf), "--min-count", str(mc)] + fw, capture_output=True)
        assert r.returncode == 0 and r.stdout == model, r.stderr
