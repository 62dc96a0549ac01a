"""GPU checks of kmc_unitigs / kmc_unitigs_device / KmerCounter.unitigs (kmc_unitig.hip.h).  Expected values come from
tests/unitig_model.py -- the definition of include/kmc.h walked key by key on Python strings -- applied to the CPU oracle's
table of the same input.  All comparisons are exact: the four arrays and the eight summary words, through every form of
the call."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import graph_model as gm
import unitig_model as um
from conftest import ROOT, SAMPLE

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "bin", "k-mer-count")
U64 = np.uint64


def _table_dict(t):
    km = t.kmers()
    return {km[i].tobytes().decode(): int(t.count[i]) for i in range(t.n_distinct)}


def _pack(reads):
    bases = np.frombuffer("".join(reads).encode(), np.uint8)
    offs = np.zeros(len(reads) + 1, U64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return bases, offs


def _dev_bytes(ptr, n):
    """n bytes at a device address (read as whole 64-bit words: the ctx's arrays are allocated with room to spare)"""
    if not n:
        return np.zeros(0, np.uint8)
    kd = importlib.import_module("k-mer-count_amd.distributed")
    import torch
    return kd.device_view(ptr, (n + 7) // 8, torch.device("cuda", 0)).cpu().numpy().view(np.uint8)[:n].copy()


def _dev_u64(ptr, n):
    return _dev_bytes(ptr, 8 * n).view(U64)


def _want_arrays(u):
    return (np.frombuffer(u.bases.encode(), np.uint8), np.array(u.offsets, U64), np.array(u.abund, U64), np.array(u.flags, np.uint8))


def _raw(kmc, kc, lo, hi, nu, nb, spare=3):
    """kmc_unitigs through ctypes into arrays with `spare` entries more than needed, filled with a pattern"""
    L = kmc.lib()
    bases, flags = np.full(nb + spare, 0xEE, np.uint8), np.full(nu + spare, 0xEE, np.uint8)
    offs, abund = np.full(nu + 1 + spare, 0xEEEE, U64), np.full(nu + spare, 0xEEEE, U64)
    n1, n2 = C.c_uint64(12345), C.c_uint64(12345)
    w = (C.c_uint64 * kmc.UNITIG_WORDS)()
    kc._chk(L.kmc_unitigs(kc._h, lo, hi, bases.ctypes.data, nb + spare, offs.ctypes.data, abund.ctypes.data, flags.ctypes.data, nu + spare,
                          C.byref(n1), C.byref(n2), w))
    assert (n1.value, n2.value) == (nu, nb)
    assert (bases[nb:] == 0xEE).all() and (flags[nu:] == 0xEE).all() and (offs[nu + 1:] == 0xEEEE).all() and (abund[nu:] == 0xEEEE).all()
    return (bases[:nb], offs[:nu + 1], abund[:nu], flags[:nu]), list(w)


def _same(got, want, ctx):
    for name, g, w in zip(("bases", "offsets", "abund", "flags"), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), (ctx, name, g[:40], w[:40])


def _check(kmc, kc, table, canonical, ranges):
    """every form of the call against the model, for every range; returns {range: model words}"""
    L = kmc.lib()
    seen = {}
    for lo, hi in ranges:
        u = um.unitigs(table, canonical, lo, hi)
        want, words = _want_arrays(u), u.summary
        nu, nb = words[0], words[1]
        ctx = (kc.k, canonical, lo, hi)
        g = gm.graph(table, canonical, lo, hi)[2]
        assert words[1] == words[2] + (kc.k - 1) * words[0] and 2 * words[0] == g[6] + words[6] + 2 * words[3] and words[2] == g[0]
        # the sizing call
        n1, n2 = C.c_uint64(1), C.c_uint64(1)
        w = (C.c_uint64 * 8)()
        kc._chk(L.kmc_unitigs(kc._h, lo, hi, None, 0, None, None, None, 0, C.byref(n1), C.byref(n2), w))
        assert (n1.value, n2.value, list(w)) == (nu, nb, words), (ctx, list(w), words)
        got, w = _raw(kmc, kc, lo, hi, nu, nb)
        assert w == words, (ctx, w, words)
        _same(got, want, ctx)
        db, do, da, df, dn, dnb, s = kc.unitigs_device(lo, hi)
        assert (dn, dnb, s.words()) == (nu, nb, words) and db and do and da and df
        assert db % 16 == 0 and do % 8 == 0
        _same((_dev_bytes(db, nb), _dev_u64(do, nu + 1), _dev_u64(da, nu), _dev_bytes(df, nu)), want, ctx)
        r = kc.unitigs(lo, hi)
        _same((r.bases, r.offsets, r.abund, r.flags), want, ctx)
        assert r.summary.words() == words and r.strings() == u.seqs and r.to_fasta() == u.fasta() and len(r) == nu
        assert kc.graph(lo, hi, adj=False)[1].words() == g
        seen[(lo, hi)] = words
    return seen


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [1, 2, 4, 5, 6, 21, 31, 32, 33, 47, 63])
def test_sample_fasta(kmc, oracle, k, canonical):
    bases, offs = kmc.parse_fasta(SAMPLE)
    want = oracle.count_kmers(bases, offs, k, canonical)
    table = _table_dict(want)
    with kmc.KmerCounter(k=k, canonical=canonical) as kc:
        kc.add_batch(bases, offs)
        assert kc.export().equals(want)
        _check(kmc, kc, table, canonical, ((1, 0), (2, 0), (3, 6)))


def _rnd(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def _constructed(k, seed, few=False):
    """The reads of the graph test -- random reads of lengths k, k + 1, k + 5, 150 and 400, each one to three times; a fork,
    twice; a read with an N; the other strand of a stretch of a long read; a homopolymer; an AT repeat -- and circular
    ones: s + s[:k + 2] for a random s of 100 and of 2 bases; for even k a palindromic k-mer between the two k-mers that are
    each other's reverse complement (two of its sides claim one partner).
    few: the same shapes in some sixty k-mers -- three short random reads, a fork of k + 9 bases, the homopolymer, the AT
    repeat, circular reads of 12 and of 2 bases, the palindrome -- for a k whose k-mer space the full set nearly fills."""
    rng = np.random.default_rng(seed)
    reads = []
    if few:
        for n in (k, k + 1, k + 5):
            reads += [_rnd(rng, n)] * int(rng.integers(1, 4))
        stem = _rnd(rng, k + 4)
        reads += [stem + _rnd(rng, 5), stem + _rnd(rng, 5)] * 2
    else:
        for n in (k, k + 1, k + 5, 150, 400):
            for _ in range(6):
                reads += [_rnd(rng, max(n, k))] * int(rng.integers(1, 4))
        stem = _rnd(rng, 150)
        reads += [stem + _rnd(rng, 60), stem + _rnd(rng, 60)] * 2
        s = _rnd(rng, 200)
        reads.append(s[:90] + "N" + s[91:])
        long_ = [r for r in reads if len(r) == 400][0]
        reads.append(gm.revcomp(long_[100:300]))
    reads.append("A" * (k + 20))
    reads.append(("AT" * (k + 20))[: k + 31])
    for n in ((12, 2) if few else (100, 2)):
        s = _rnd(rng, n)
        reads += [(s * (k + 2))[:n + k + 2]] * 2
    if k % 2 == 0:
        half = _rnd(rng, k // 2)
        reads.append("G" + half + gm.revcomp(half) + "C")
    return reads


def _check_reads(kmc, oracle, reads, k, canonical):
    bases, offs = _pack(reads)
    want = oracle.count_kmers(bases, offs, k, canonical)
    table = _table_dict(want)
    assert table == gm.count_table(reads, k, canonical)
    with kmc.KmerCounter(k=k, canonical=canonical) as kc:
        kc.add_batch(bases, offs)
        assert kc.export().equals(want)
        seen = _check(kmc, kc, table, canonical, ((1, 0), (2, 0), (1, 1), (2, 3)))
    assert any(w[2] < len(table) for w in seen.values()), seen
    return seen


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [6, 21, 31, 32, 33, 63])
def test_constructed_and_circular_reads(kmc, oracle, k, canonical):
    seen = _check_reads(kmc, oracle, _constructed(k, 500 + k), k, canonical)
    # What makes this input worth having: a range with circular, one-key and multi-key unitigs and unjoined sides at once.
    # At k = 6 the full set nearly fills the space of 6-mers and no cycle survives the branching, so it checks exactness
    # alone there and the few reads of the same shapes carry the assertion.
    rich = seen if k >= 21 else _check_reads(kmc, oracle, _constructed(k, 500 + k, few=True), k, canonical)
    # Unjoined sides need a canonical ctx: in a forward one the partner of (x, R) is (y, L), whose one left neighbour is x
    # again, so every side that continues is joined and [6] is 0 whatever the input.
    assert any(w[3] and w[4] and w[5] > 1 and (w[6] or not canonical) for w in rich.values()), rich
    if not canonical:
        assert all(w[6] == 0 for w in list(seen.values()) + list(rich.values())), (seen, rich)


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("closed", [False, True])
def test_ranking_depth(kmc, oracle, canonical, closed):
    """one unitig of 69 970 keys: 17 doubling rounds, past any batch of rounds between two looks of the host; and the same
    read closed into a cycle"""
    k = 31
    s = _rnd(np.random.default_rng(7), 70_000)
    read = s + s[:k - 1] if closed else s
    bases, offs = _pack([read])
    want = oracle.count_kmers(bases, offs, k, canonical)
    table = _table_dict(want)
    assert len(table) == (70_000 if closed else 69_970)
    with kmc.KmerCounter(k=k, canonical=canonical) as kc:
        kc.add_batch(bases, offs)
        assert kc.export().equals(want)
        seen = _check(kmc, kc, table, canonical, ((1, 0),))
    assert seen[(1, 0)][0] == 1 and seen[(1, 0)][3] == (1 if closed else 0) and seen[(1, 0)][5] == len(table)


@pytest.mark.parametrize("k,canonical", [(31, True), (31, False), (63, True)])
def test_table_of_many_workgroups(kmc, oracle, k, canonical):
    n_reads = 640
    sb, so = kmc.synth_reads_host(kmc.Synth(seed=31, pool=0), 0, n_reads)     # 400-base reads, every line fresh random
    bases = np.concatenate([sb, sb[:int(so[150])]])                            # the first 150 reads twice: counts of 2
    offs = np.concatenate([so, so[1:151] + so[-1]])
    want = oracle.count_kmers(bases, offs, k, canonical, method=1)
    assert want.n_distinct >= 200_000
    table = _table_dict(want)
    with kmc.KmerCounter(k=k, canonical=canonical) as kc:
        kc.add_batch(bases, offs)
        assert kc.export().equals(want)
        seen = _check(kmc, kc, table, canonical, ((1, 0), (2, 0)))
    assert seen[(1, 0)][2] == want.n_distinct and 0 < seen[(2, 0)][2] < want.n_distinct


@pytest.mark.parametrize("canonical", [True, False])
def test_round_trip_on_the_device(kmc, oracle, canonical):
    """the unitigs of one ctx counted by another, no host copy: every solid key exactly once"""
    reads = _constructed(31, 77)
    bases, offs = _pack(reads)
    with kmc.KmerCounter(k=31, canonical=canonical) as kc, kmc.KmerCounter(k=31, canonical=canonical) as other:
        kc.add_batch(bases, offs)
        kc.finalize()
        for lo, hi in ((1, 0), (2, 0)):
            db, do, _, _, nu, nb, s = kc.unitigs_device(lo, hi)
            other.reset()
            other.add_batch_device(db, do, nu, nb, 0)
            got = other.export()
            want = kc.export_filtered(lo, hi)
            assert s.keys == want.n_distinct > 0
            assert np.array_equal(got.key_lo, want.key_lo) and np.array_equal(got.key_hi, want.key_hi)
            assert (got.count == 1).all()


def test_state_and_errors(kmc, oracle):
    L = kmc.lib()
    bases, offs = kmc.parse_fasta(SAMPLE)
    half = len(offs) // 2
    b1, o1 = bases[:int(offs[half])], offs[:half + 1]
    t1 = _table_dict(oracle.count_kmers(b1, o1, 31, True))
    t2 = _table_dict(oracle.count_kmers(bases, offs, 31, True))
    n1, n2 = C.c_uint64(99), C.c_uint64(99)
    w = (C.c_uint64 * 8)(*([7] * 8))
    p = [C.c_void_p(1) for _ in range(4)]

    def host(kc, lo, hi):
        return L.kmc_unitigs(kc._h, lo, hi, None, 0, None, None, None, 0, C.byref(n1), C.byref(n2), w)

    def device(kc, lo, hi):
        return L.kmc_unitigs_device(kc._h, lo, hi, *[C.byref(x) for x in p], C.byref(n1), C.byref(n2), w)

    def state(kc):
        """what the unitig calls say in this state, checked against kmc_export"""
        rc = L.kmc_export(kc._h, None, None, None, 0)
        exp = kmc.ERR_STATE if rc == kmc.ERR_STATE else kmc.OK
        assert (host(kc, 1, 0) == kmc.ERR_STATE) == (exp == kmc.ERR_STATE)
        assert (device(kc, 1, 0) == kmc.ERR_STATE) == (exp == kmc.ERR_STATE)
        return exp

    with kmc.KmerCounter(k=31) as kc:
        assert state(kc) == kmc.ERR_STATE                    # before any finalize
        kc.add_batch(b1, o1)
        assert state(kc) == kmc.ERR_STATE
        kc.finalize()
        assert state(kc) == kmc.OK
        # every output pointer may be NULL
        assert L.kmc_unitigs_device(kc._h, 1, 0, None, None, None, None, None, None, None) == kmc.OK
        assert L.kmc_unitigs(kc._h, 1, 0, None, 0, None, None, None, 0, None, None, None) == kmc.OK
        # a bad range
        assert host(kc, 3, 2) == kmc.ERR_ARG and device(kc, 3, 2) == kmc.ERR_ARG
        assert host(kc, 3, 3) == kmc.OK
        u = um.unitigs(t1, True)
        nu, nb = u.summary[0], u.summary[1]
        assert host(kc, 1, 0) == kmc.OK and (n1.value, n2.value, list(w)) == (nu, nb, u.summary)
        # too small: the sizes are set, nothing is copied
        bases_o, flags_o = np.full(nb, 0xEE, np.uint8), np.full(nu, 0xEE, np.uint8)
        offs_o, abund_o = np.full(nu + 1, 0xEEEE, U64), np.full(nu, 0xEEEE, U64)
        for cb, cu in ((nb - 1, nu), (nb, nu - 1), (0, 0)):
            n1.value = n2.value = 0
            assert L.kmc_unitigs(kc._h, 1, 0, bases_o.ctypes.data, cb, offs_o.ctypes.data, abund_o.ctypes.data, flags_o.ctypes.data, cu,
                                 C.byref(n1), C.byref(n2), w) == kmc.ERR_ARG
            assert (n1.value, n2.value) == (nu, nb)
            assert (bases_o == 0xEE).all() and (flags_o == 0xEE).all() and (offs_o == 0xEEEE).all() and (abund_o == 0xEEEE).all()
        # one array alone
        assert L.kmc_unitigs(kc._h, 1, 0, None, 0, None, abund_o.ctypes.data, None, nu, C.byref(n1), C.byref(n2), None) == kmc.OK
        assert np.array_equal(abund_o, np.array(u.abund, U64)) and (offs_o == 0xEEEE).all()
        _check(kmc, kc, t1, True, ((1, 0),))
        # more batches, a second finalize: the new unitigs, not the old index or buffers
        kc.add_batch(bases[int(offs[half]):], offs[half:] - offs[half])
        assert state(kc) == kmc.ERR_STATE                    # the view is stale
        kc.finalize()
        _check(kmc, kc, t2, True, ((1, 0), (2, 0)))
        kc.reset()
        assert state(kc) == kmc.ERR_STATE
        # an empty view: zeros
        kc.finalize()
        r = kc.unitigs()
        assert len(r) == 0 and r.bases.shape == (0,) and list(r.offsets) == [0] and r.summary.words() == [0] * 8 and r.to_fasta() == ""
        d = kc.unitigs_device()
        assert d[4:6] == (0, 0) and d[6].words() == [0] * 8
    with kmc.KmerCounter(k=31) as kc:     # reads shorter than k: an empty view too
        kc.add_batch(*_pack(["ACGTACGT", "TTTT", "A" * 30]))
        kc.finalize()
        n1.value = 5
        assert host(kc, 1, 0) == kmc.OK and n1.value == 0 and n2.value == 0 and list(w) == [0] * 8
    with kmc.KmerCounter(k=31) as kc:     # a range that no key is in
        kc.add_batch(b1, o1)
        kc.finalize()
        r = kc.unitigs(10 ** 9, 0)
        assert len(r) == 0 and list(r.offsets) == [0] and r.summary.words() == [0] * 8
    with kmc.KmerCounter(mode=kmc.MODE_LR) as kc:
        kc.count_file(SAMPLE)
        kc.finalize()
        assert host(kc, 1, 0) == kmc.ERR_ARG and device(kc, 1, 0) == kmc.ERR_ARG
        with pytest.raises(kmc.KmcError) as e:
            kc.unitigs()
        assert e.value.status == kmc.ERR_ARG


def test_host_form_copies_a_kept_result_only_of_its_view_and_range(kmc, oracle):
    """kmc_unitigs after a call for the same view and range copies that call's result; another range, a graph call in
    between or a new view must not leave it with the wrong one"""
    bases, offs = kmc.parse_fasta(SAMPLE)
    half = len(offs) // 2
    b1, o1 = bases[:int(offs[half])], offs[:half + 1]
    full = _table_dict(oracle.count_kmers(bases, offs, 31, True))
    part = _table_dict(oracle.count_kmers(b1, o1, 31, True))

    def host_is(kc, table, lo, hi):
        u = um.unitigs(table, True, lo, hi)
        got, w = _raw(kmc, kc, lo, hi, u.summary[0], u.summary[1])
        assert w == u.summary
        _same(got, _want_arrays(u), (lo, hi))

    with kmc.KmerCounter(k=31) as kc:
        kc.add_batch(bases, offs)
        kc.finalize()
        kc.unitigs_device(1, 0)
        host_is(kc, full, 2, 0)              # another range than the kept one
        host_is(kc, full, 2, 0)              # the kept one
        kc.unitigs_device(1, 0)
        kc.graph_device(2, 0)                # rewrites adj, not the unitig arrays
        host_is(kc, full, 1, 0)
        host_is(kc, full, 1, 3)
        kc.reset()
        kc.add_batch(b1, o1)
        kc.finalize()
        host_is(kc, part, 1, 3)              # the same range on a new view
        kc.reset()
        kc.finalize()
        host_is(kc, {}, 1, 3)                # and on an empty one


def test_after_finalize_async(kmc, oracle):
    hb, ho = kmc.synth_reads_host(kmc.Synth(seed=4), 0, 3000)
    want = oracle.count_kmers(hb, ho, 31, True)
    u = um.unitigs(_table_dict(want), True, 2, 0)
    arrays = _want_arrays(u)
    for form in ("unitigs", "unitigs_device"):
        with kmc.KmerCounter(k=31) as kc:
            kc.add_batch(hb, ho)
            kc.export()
            kc.reset()
            kc.add_batch(hb, ho)
            ok0 = kc.stats().n_async_ok
            kc.finalize_async()          # a view queued and never observed before the unitig call
            if form == "unitigs":
                r = kc.unitigs(2, 0)
                got, words = (r.bases, r.offsets, r.abund, r.flags), r.summary.words()
            else:
                db, do, da, df, nu, nb, s = kc.unitigs_device(2, 0)
                got, words = (_dev_bytes(db, nb), _dev_u64(do, nu + 1), _dev_u64(da, nu), _dev_bytes(df, nu)), s.words()
            _same(got, arrays, form)
            assert words == u.summary
            assert kc.finalize() == (want.n_distinct, want.n_total)
            assert kc.stats().n_async_ok == ok0 + 1


def test_nothing_else_moved(kmc, oracle):
    bases, offs = kmc.parse_fasta(SAMPLE)
    half = len(offs) // 2
    for k in (31, 63):
        want = oracle.count_kmers(bases, offs, k, True)
        table = _table_dict(want)
        rng = np.random.default_rng(k)
        qlo = np.concatenate([want.key_lo, want.key_lo ^ U64(1)])
        qhi = np.concatenate([want.key_hi, want.key_hi])
        p = rng.permutation(len(qlo))
        qlo, qhi = qlo[p], qhi[p]
        with kmc.KmerCounter(k=k) as kc, kmc.KmerCounter(k=k) as other:
            kc.add_batch(bases, offs)
            kc.finalize()
            other.add_batch(bases[:int(offs[half])], offs[:half + 1])
            other.finalize()
            digest = kc.export().digest()
            vp = kc.export_device()
            fhi, flo, fcnt, nk, _ = kc.filter_device(2, 0)
            shi, slo, scnt, ns, _ = kc.setop_device(other, "subtract")
            pb, phi, plo, pcnt = kc.partition_device(4)
            n = pb[-1]
            arrays = ((plo, n), (pcnt, n), (flo, nk), (fcnt, nk), (slo, ns), (scnt, ns))
            before = [_dev_u64(ptr, m) for ptr, m in arrays]
            q_before = kc.query(qlo, qhi)                     # builds the index
            assert q_before.any() and not q_before.all()
            _check(kmc, kc, table, True, ((1, 0), (2, 0)))    # reuses it
            after = [_dev_u64(ptr, m) for ptr, m in arrays]
            assert all(np.array_equal(a, b) for a, b in zip(before, after))
            assert kc.export_device() == vp and kc.export().digest() == digest
            assert np.array_equal(kc.query(qlo, qhi), q_before)
        # the other order: the unitig call builds the index, the query reuses it
        with kmc.KmerCounter(k=k) as kc:
            kc.add_batch(bases, offs)
            kc.finalize()
            _check(kmc, kc, table, True, ((1, 0),))
            assert np.array_equal(kc.query(qlo, qhi), q_before)
            _check(kmc, kc, table, True, ((2, 3),))


@pytest.mark.parametrize("forward", [False, True])
@pytest.mark.parametrize("k", [31, 63])
def test_cli_unitigs(kmc, oracle, k, forward):
    bases, offs = kmc.parse_fasta(SAMPLE)
    table = _table_dict(oracle.count_kmers(bases, offs, k, not forward))
    fw = ["--forward"] if forward else []
    for rng_args, (lo, hi) in (([], (1, 0)), (["--min-count", "3"], (3, 0)), (["--min-count", "2", "--max-count", "4"], (2, 4))):
        r = subprocess.run([EXE, SAMPLE, "-k", str(k), "--unitigs"] + rng_args + fw, capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout == um.unitigs(table, not forward, lo, hi).fasta(), r.stderr
