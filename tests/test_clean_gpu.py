"""GPU checks of kmc_unitig_clean / kmc_unitig_clean_device / kmc_unitig_clean_into and KmerCounter.clean_unitigs / cleaned
(kmc_clean.hip.h).  Expected values come from tests/clean_model.py -- the definition of include/kmc.h on the unitigs and
links of unitig_model.py / links_model.py -- applied to the CPU oracle's table of the same input.  All comparisons are exact:
the verdicts, the kept table in view order and the eight summary words, through every form of the call."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import clean_inputs as ci
import clean_model as cm
import graph_model as gm
import links_model as lm
import unitig_model as um
from conftest import ROOT, SAMPLE
from test_links_gpu import _branching, _dev_u32
from test_unitig_gpu import _dev_bytes, _dev_u64, _pack, _same, _table_dict, _want_arrays

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "bin", "k-mer-count")
U64, U8 = np.uint64, np.uint8
RANGES = ((1, 0), (2, 0), (1, 1), (2, 3))
BIG = 1 << 31


def _limits(k):
    return ((k, k), (0, 0), (1, 1), (BIG, BIG), (k, 0), (0, k))


def _want(kmc, c):
    """(key_hi, key_lo, count, verdict) of a model result, the kept keys in view order"""
    keys = sorted(c.kept)
    enc = [kmc.encode_key(x, False) for x in keys]
    return (np.array([e[0] for e in enc], U64), np.array([e[1] for e in enc], U64), np.array([c.kept[x] for x in keys], U64),
            np.array(c.verdict, U8))


def _equal(got, want, ctx):
    for name, g, w in zip(("key_hi", "key_lo", "count", "verdict"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (ctx, name, g[:20], w[:20])


def _raw(kmc, kc, lo, hi, tip, isl, nk, nu, spare=3):
    """kmc_unitig_clean through ctypes into arrays with `spare` entries more than needed, filled with a pattern"""
    L = kmc.lib()
    a = [np.full(nk + spare, 0xEEEE, U64) for _ in range(3)]
    v = np.full(nu + spare, 0xEE, U8)
    n1, n2 = C.c_uint64(12345), C.c_uint64(12345)
    w = (C.c_uint64 * kmc.CLEAN_WORDS)()
    kc._chk(L.kmc_unitig_clean(kc._h, lo, hi, tip, isl, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, nk + spare, v.ctypes.data, nu + spare,
                               C.byref(n1), C.byref(n2), w))
    assert (n1.value, n2.value) == (nk, nu)
    assert all((x[nk:] == 0xEEEE).all() for x in a) and (v[nu:] == 0xEE).all()
    return (a[0][:nk], a[1][:nk], a[2][:nk], v[:nu]), list(w)


def _check(kmc, kc, table, canonical, ranges, limits):
    """every form of the call against the model, for every range and pair of limits; returns {(range, limits): the model's Clean}"""
    L = kmc.lib()
    seen = {}
    for lo, hi in ranges:
        graph = (um.unitigs(table, canonical, lo, hi), lm.links(table, canonical, lo, hi))
        for tip, isl in limits:
            c = cm.clean(table, canonical, lo, hi, tip, isl, graph=graph)
            want, words = _want(kmc, c), c.summary
            nk, nu = words[3], words[0]
            ctx = (kc.k, canonical, lo, hi, tip, isl)
            assert words[3] + words[4] + words[5] == graph[0].summary[2]
            # the sizing call
            n1, n2 = C.c_uint64(1), C.c_uint64(1)
            w = (C.c_uint64 * 8)()
            kc._chk(L.kmc_unitig_clean(kc._h, lo, hi, tip, isl, None, None, None, 0, None, 0, C.byref(n1), C.byref(n2), w))
            assert (n1.value, n2.value, list(w)) == (nk, nu, words), (ctx, list(w), words)
            got, w = _raw(kmc, kc, lo, hi, tip, isl, nk, nu)
            assert w == words, (ctx, w, words)
            _equal(got, want, ctx)
            # the device form, read back
            dh, dl, dc, dv, dnk, dnu, s = kc.clean_unitigs_device(lo, hi, tip, isl)
            assert (dnk, dnu, s.words()) == (nk, nu, words), (ctx, s.words(), words)
            assert dl and dc and dv and dl % 8 == 0 and dc % 8 == 0 and bool(dh) == (kc.k > 31)
            g_hi = _dev_u64(dh, nk) if dh else np.zeros(nk, U64)
            _equal((g_hi, _dev_u64(dl, nk), _dev_u64(dc, nk), _dev_bytes(dv, nu)), want, ctx)
            r = kc.clean_unitigs(lo, hi, tip, isl)
            _equal((r.table.key_hi, r.table.key_lo, r.table.count, r.verdict), want, ctx)
            assert r.summary.words() == words and r.table.n_distinct == nk
            if (tip, isl) == (0, 0):
                assert r.table.equals(kc.export_filtered(lo, hi)), ctx
            seen[((lo, hi), (tip, isl))] = c
        # the summary identity, on the library's own words
        t = kc.unitigs(lo, hi).summary.words()
        s = kc.clean_unitigs(lo, hi).summary.words()
        assert s[3] + s[4] + s[5] == t[2] and s[0] == t[0]
    return seen


def _counter(kmc, oracle, reads, k, canonical):
    bases, offs = _pack(reads)
    want = oracle.count_kmers(bases, offs, k, canonical)
    table = _table_dict(want)
    assert table == gm.count_table(reads, k, canonical)
    kc = kmc.KmerCounter(k=k, canonical=canonical)
    kc.add_batch(bases, offs)
    assert kc.export().equals(want)
    return kc, table


def _merged(kmc, table, k, canonical):
    """a finalized counter whose table is exactly {k-mer: count}, through kmc_merge_pairs_device"""
    import torch
    keys = list(table)
    enc = [kmc.encode_key(x, False) for x in keys]
    dev = lambda a: torch.tensor(np.array(a, U64).view(np.int64), device="cuda")
    d_hi, d_lo, d_cnt = dev([e[0] for e in enc]), dev([e[1] for e in enc]), dev([table[x] for x in keys])
    kc = kmc.KmerCounter(k=k, canonical=canonical)
    kc.merge_pairs_device(d_hi.data_ptr() if k > 31 else 0, d_lo.data_ptr(), d_cnt.data_ptr(), len(keys))
    assert kc.finalize()[0] == len(keys)
    torch.cuda.synchronize()
    assert _table_dict(kc.export()) == table
    return kc


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [1, 2, 4, 5, 6, 21, 31, 32, 33, 47, 63])
def test_sample_fasta(kmc, oracle, k, canonical):
    bases, offs = kmc.parse_fasta(SAMPLE)
    want = oracle.count_kmers(bases, offs, k, canonical)
    with kmc.KmerCounter(k=k, canonical=canonical) as kc:
        kc.add_batch(bases, offs)
        assert kc.export().equals(want)
        _check(kmc, kc, _table_dict(want), canonical, RANGES, _limits(k))


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [6, 21, 32, 33, 63])
def test_branching_reads(kmc, oracle, k, canonical):
    """hairpins, palindromes for even k, dropped records, circular unitigs (all kept), with limits 3k"""
    kc, table = _counter(kmc, oracle, _branching(k, 900 + k), k, canonical)
    with kc:
        seen = _check(kmc, kc, table, canonical, ((1, 0), (2, 0)), ((3 * k, 3 * k),))
    c = seen[((1, 0), (3 * k, 3 * k))]
    assert all(c.verdict[u] == cm.KEEP for u, f in enumerate(c.unitigs.flags) if f)
    if k >= 21:
        assert sum(c.unitigs.flags) > 0
        assert c.summary[6] == 6 and c.summary[1] == 3, c.summary


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [21, 32, 33])
def test_forks_and_islands(kmc, oracle, k, canonical):
    reads = ci.five_forks(k, 100 + k)[0] + ci.islands(k, 200 + k)
    kc, table = _counter(kmc, oracle, reads, k, canonical)
    with kc:
        seen = _check(kmc, kc, table, canonical, ((1, 0),), _limits(k) + ((0, k + 1),))
    assert seen[((1, 0), (k, k))].summary[:3] == [18, 6, 1] and seen[((1, 0), (k, k))].summary[6] == 9
    assert seen[((1, 0), (0, k + 1))].summary[:3] == [18, 0, 2]


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [21, 32, 33])
def test_wide_products(kmc, k, canonical):
    """mean abundances whose comparison needs more than 64 bits of product"""
    table, arm5, arm6 = ci.wide_fork(k, canonical, 300 + k)
    with _merged(kmc, table, k, canonical) as kc:
        seen = _check(kmc, kc, table, canonical, ((1, 0),), ((k, k),))
    c = seen[((1, 0), (k, k))]
    u5, u6 = ci.unitig_of(c.unitigs, arm5, k, canonical), ci.unitig_of(c.unitigs, arm6, k, canonical)
    assert (c.verdict[u5], c.verdict[u6]) == (cm.TIP, cm.KEEP)


def test_nothing_solid_and_empty_view(kmc, oracle):
    bases, offs = kmc.parse_fasta(SAMPLE)
    with kmc.KmerCounter(k=31) as kc:
        kc.add_batch(bases, offs)
        kc.finalize()
        r = kc.clean_unitigs(10 ** 9, 0)
        assert r.table.n_distinct == 0 and r.verdict.shape == (0,) and r.summary.words() == [0] * 8
        d = kc.clean_unitigs_device(10 ** 9, 0)
        assert d[4:6] == (0, 0) and d[6].words() == [0] * 8 and d[1] and d[2] and d[3]
        kc.reset()
        kc.finalize()
        r = kc.clean_unitigs()
        assert r.table.n_distinct == 0 and r.verdict.shape == (0,) and r.summary.words() == [0] * 8
        d = kc.clean_unitigs_device()
        assert d[4:6] == (0, 0) and d[6].words() == [0] * 8
        with kmc.KmerCounter(k=31) as dst:
            assert kc.clean_into(dst).words() == [0] * 8
            assert dst.finalize() == (0, 0)


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [21, 32, 33])
def test_clean_into_and_cleaned_rounds(kmc, oracle, k, canonical):
    reads = ci.rounds_input(k, 400 + k)
    kc, table = _counter(kmc, oracle, reads, k, canonical)
    with kc:
        digest = kc.export().digest()
        for lo, hi in ((1, 0), (2, 0)):
            final, words = cm.rounds(table, canonical, lo, hi, n_rounds=4)
            out, got = kc.cleaned(lo, hi, rounds=4)
            with out:
                assert [s.words() for s in got] == words and len(got) == len(words)
                assert (out.k, out.canonical, out.device) == (kc.k, kc.canonical, kc.device)
                assert _table_dict(out.export()) == final
                u, lk = um.unitigs(final, canonical, lo, hi), lm.links(final, canonical, lo, hi)
                r = out.unitigs(lo, hi)
                _same((r.bases, r.offsets, r.abund, r.flags), _want_arrays(u), (k, canonical, lo, hi))
                assert r.summary.words() == u.summary
                l = out.unitig_links(lo, hi)
                assert np.array_equal(l.offsets, np.array(lk.offsets, U64)) and np.array_equal(l.to, np.array(lk.to, np.uint32))
                assert l.summary.words() == lk.summary
            if (lo, hi) == (1, 0):
                assert len(words) == 2 and sorted(len(s) - k + 1 for s in u.seqs) == sorted([5 * k + 1, k + 6])
        # one round, by hand
        one, w1 = cm.rounds(table, canonical, n_rounds=1)
        out, got = kc.cleaned(rounds=1)
        with out:
            assert [s.words() for s in got] == w1 and _table_dict(out.export()) == one
        assert kc.export().digest() == digest               # the source is as it was
        # two sources into one dst: the counts of the keys both keep add up
        other_reads = ci.five_forks(k, 100 + k)[0] + reads[:3]
        kc2, table2 = _counter(kmc, oracle, other_reads, k, canonical)
        with kc2, kmc.KmerCounter(k=k, canonical=canonical) as dst:
            s1, s2 = kc.clean_into(dst), kc2.clean_into(dst)
            c1, c2 = cm.clean(table, canonical), cm.clean(table2, canonical)
            assert s1.words() == c1.summary and s2.words() == c2.summary
            both = dict(c1.kept)
            for x, n in c2.kept.items():
                both[x] = both.get(x, 0) + n
            assert _table_dict(dst.export()) == both and len(both) < len(c1.kept) + len(c2.kept)


_CHILD = r"""
import importlib, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
kmc = importlib.import_module("k-mer-count_amd")
bases, offs = kmc.parse_fasta(sys.argv[2])
with kmc.KmerCounter(k=31) as kc:
    kc.add_batch(bases, offs)
    kc.finalize()
    print("step links(1,0)", file=sys.stderr, flush=True)
    kc.unitig_links(1, 0)
    print("step clean(1,0)", file=sys.stderr, flush=True)
    a = kc.clean_unitigs(1, 0)
    print("step clean(1,0) again", file=sys.stderr, flush=True)
    b = kc.clean_unitigs(1, 0)
    assert a.table.equals(b.table)
    print("step clean(1,0) other limits", file=sys.stderr, flush=True)
    kc.clean_unitigs(1, 0, 5, 5)
    print("step clean_device(1,0)", file=sys.stderr, flush=True)
    kc.clean_unitigs_device(1, 0)
    print("step graph(2,0) clean(1,0)", file=sys.stderr, flush=True)
    kc.graph(2, 0, adj=False)
    kc.clean_unitigs_device(1, 0)
    print("step clean(2,0)", file=sys.stderr, flush=True)
    kc.clean_unitigs(2, 0)
    print("step end", file=sys.stderr, flush=True)
"""


def test_clean_reuses_the_held_unitigs_and_links(kmc):
    """What computes, seen through the KMC_UNITIG_TRACE lines of a child process (nothing is timed)"""
    env = dict(os.environ, KMC_UNITIG_TRACE="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, SAMPLE], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    steps, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("step "):
            cur = line[5:]
            steps[cur] = []
        elif line.split(":")[0] in ("kmc_unitigs", "kmc_unitig_links", "kmc_unitig_clean"):
            steps[cur].append(line.split(":")[0])
    assert steps["links(1,0)"] == ["kmc_unitigs", "kmc_unitig_links"]
    # behind the links of the same range: neither a unitigs nor a links line, and sizing then copy is one clean pass
    assert steps["clean(1,0)"] == ["kmc_unitig_clean"]
    assert steps["clean(1,0) again"] == []
    assert steps["clean(1,0) other limits"] == ["kmc_unitig_clean"]
    # the device form always runs the clean pass
    assert steps["clean_device(1,0)"] == ["kmc_unitig_clean"]
    # a graph call has rewritten adj: both are computed again
    assert steps["graph(2,0) clean(1,0)"] == ["kmc_unitigs", "kmc_unitig_links", "kmc_unitig_clean"]
    assert steps["clean(2,0)"] == ["kmc_unitigs", "kmc_unitig_links", "kmc_unitig_clean"]
    assert "clean_ms" in r.stderr


def test_nothing_else_moved(kmc, oracle):
    bases, offs = kmc.parse_fasta(SAMPLE)
    half = len(offs) // 2
    for k in (31, 63):
        want = oracle.count_kmers(bases, offs, k, True)
        table = _table_dict(want)
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
            db, do, da, df, nu, nb, _ = kc.unitigs_device(2, 0)
            lo_, lt, lnu, nl, _ = kc.unitig_links_device(2, 0)
            arrays = ((plo, n), (pcnt, n), (flo, nk), (fcnt, nk), (slo, ns), (scnt, ns), (do, nu + 1), (da, nu), (lo_, 2 * nu + 1))
            read = lambda: [_dev_u64(ptr, m) for ptr, m in arrays] + [_dev_bytes(db, nb), _dev_bytes(df, nu), _dev_u32(lt, nl)]
            before = read()
            q = np.concatenate([want.key_lo, want.key_lo ^ U64(1)])
            qh = np.concatenate([want.key_hi, want.key_hi])
            q_before = kc.query(q, qh)
            _check(kmc, kc, table, True, ((2, 0),), ((k, k), (0, 0)))     # on the unitigs and links the ctx holds
            after = read()
            assert all(np.array_equal(a, b) for a, b in zip(before, after))
            u, lk = um.unitigs(table, True, 2, 0), lm.links(table, True, 2, 0)
            _same((after[9], after[6], after[7], after[10]), _want_arrays(u), k)
            assert np.array_equal(after[8], np.array(lk.offsets, U64)) and np.array_equal(after[11], np.array(lk.to, np.uint32))
            assert kc.export_device() == vp and kc.export().digest() == digest
            assert np.array_equal(kc.query(q, qh), q_before)


def test_state_and_errors(kmc, oracle):
    L = kmc.lib()
    bases, offs = kmc.parse_fasta(SAMPLE)
    table = _table_dict(oracle.count_kmers(bases, offs, 31, True))
    n1, n2 = C.c_uint64(99), C.c_uint64(99)
    w = (C.c_uint64 * 8)(*([7] * 8))
    p = [C.c_void_p(1) for _ in range(4)]

    def host(kc, lo, hi):
        return L.kmc_unitig_clean(kc._h, lo, hi, 31, 31, None, None, None, 0, None, 0, C.byref(n1), C.byref(n2), w)

    def device(kc, lo, hi):
        return L.kmc_unitig_clean_device(kc._h, lo, hi, 31, 31, *[C.byref(x) for x in p], C.byref(n1), C.byref(n2), w)

    assert L.kmc_unitig_clean(None, 1, 0, 31, 31, None, None, None, 0, None, 0, None, None, None) == kmc.ERR_ARG
    with kmc.KmerCounter(k=31) as kc, kmc.KmerCounter(k=31) as dst:
        assert host(kc, 1, 0) == kmc.ERR_STATE and device(kc, 1, 0) == kmc.ERR_STATE          # before any finalize
        assert L.kmc_unitig_clean_into(kc._h, dst._h, 1, 0, 31, 31, None) == kmc.ERR_STATE
        kc.add_batch(bases, offs)
        assert host(kc, 1, 0) == kmc.ERR_STATE and device(kc, 1, 0) == kmc.ERR_STATE
        kc.finalize()
        # every output pointer may be NULL
        assert L.kmc_unitig_clean_device(kc._h, 1, 0, 31, 31, None, None, None, None, None, None, None) == kmc.OK
        assert L.kmc_unitig_clean(kc._h, 1, 0, 31, 31, None, None, None, 0, None, 0, None, None, None) == kmc.OK
        # a bad range
        assert host(kc, 3, 2) == kmc.ERR_ARG and device(kc, 3, 2) == kmc.ERR_ARG
        assert L.kmc_unitig_clean_into(kc._h, dst._h, 3, 2, 31, 31, None) == kmc.ERR_ARG
        assert host(kc, 3, 3) == kmc.OK
        c = cm.clean(table, True)
        nk, nu = c.summary[3], c.summary[0]
        assert host(kc, 1, 0) == kmc.OK and (n1.value, n2.value, list(w)) == (nk, nu, c.summary)
        # caps one too small: the sizes are set, nothing is copied
        a = [np.full(nk, 0xEEEE, U64) for _ in range(3)]
        v = np.full(nu, 0xEE, U8)
        for ck, cu in ((nk - 1, nu), (nk, nu - 1), (0, 0)):
            n1.value = n2.value = 0
            assert L.kmc_unitig_clean(kc._h, 1, 0, 31, 31, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, ck, v.ctypes.data, cu,
                                      C.byref(n1), C.byref(n2), w) == kmc.ERR_ARG
            assert (n1.value, n2.value) == (nk, nu)
            assert all((x == 0xEEEE).all() for x in a) and (v == 0xEE).all()
        # one array alone: the cap of the ones that are NULL is not looked at
        assert L.kmc_unitig_clean(kc._h, 1, 0, 31, 31, None, None, None, 0, v.ctypes.data, nu, None, None, None) == kmc.OK
        assert np.array_equal(v, np.array(c.verdict, U8)) and all((x == 0xEEEE).all() for x in a)
        assert L.kmc_unitig_clean(kc._h, 1, 0, 31, 31, None, a[1].ctypes.data, None, nk, None, 0, None, None, None) == kmc.OK
        assert np.array_equal(a[1], _want(kmc, c)[1]) and (a[0] == 0xEEEE).all() and (a[2] == 0xEEEE).all()
        # kmc_unitig_clean_into: dst must be another ctx of the same kind
        assert L.kmc_unitig_clean_into(kc._h, kc._h, 1, 0, 31, 31, None) == kmc.ERR_ARG
        assert L.kmc_unitig_clean_into(kc._h, None, 1, 0, 31, 31, None) == kmc.ERR_ARG
        assert L.kmc_unitig_clean_into(None, dst._h, 1, 0, 31, 31, None) == kmc.ERR_ARG
        for kw in (dict(k=33), dict(k=31, canonical=False)):
            with kmc.KmerCounter(**kw) as bad:
                assert L.kmc_unitig_clean_into(kc._h, bad._h, 1, 0, 31, 31, None) == kmc.ERR_ARG
                assert b"differ in" in L.kmc_last_error(kc._h)
                with pytest.raises(kmc.KmcError) as e:
                    kc.clean_into(bad)
                assert e.value.status == kmc.ERR_ARG
        assert dst.finalize() == (0, 0)                      # nothing reached dst through the failed calls
        kc.reset()
        assert host(kc, 1, 0) == kmc.ERR_STATE and device(kc, 1, 0) == kmc.ERR_STATE
    with kmc.KmerCounter(mode=kmc.MODE_LR) as kc, kmc.KmerCounter(mode=kmc.MODE_LR) as dst:
        kc.count_file(SAMPLE)
        kc.finalize()
        assert host(kc, 1, 0) == kmc.ERR_ARG and device(kc, 1, 0) == kmc.ERR_ARG
        assert L.kmc_unitig_clean_into(kc._h, dst._h, 1, 0, 31, 31, None) == kmc.ERR_ARG
        with pytest.raises(kmc.KmcError) as e:
            kc.clean_unitigs()
        assert e.value.status == kmc.ERR_ARG


@pytest.mark.parametrize("forward", [False, True])
def test_cli_clean(kmc, tmp_path, forward):
    k = 21
    reads = ci.rounds_input(k, 400 + k)
    fa = tmp_path / "rounds.fasta"
    fa.write_text("".join(">r%d\n%s\n" % (i, s) for i, s in enumerate(reads)))
    table = gm.count_table(reads, k, not forward)
    fw = ["--forward"] if forward else []
    run = lambda *a: subprocess.run([EXE, str(fa), "-k", str(k)] + list(a) + fw, capture_output=True, text=True)
    one, w1 = cm.rounds(table, not forward, n_rounds=1)
    final, w3 = cm.rounds(table, not forward, n_rounds=3)
    r = run("--clean", "1", "--unitigs")
    assert r.returncode == 0 and r.stdout == um.unitigs(one, not forward).fasta(), r.stderr
    r = run("--clean", "3", "--gfa", "--stats")
    assert r.returncode == 0 and r.stdout == lm.gfa(um.unitigs(final, not forward), lm.links(final, not forward), k), r.stderr
    lines = [l for l in r.stderr.splitlines() if l.startswith("clean round ")]
    assert len(lines) == len(w3) == 2
    for i, (line, w) in enumerate(zip(lines, w3)):
        f = line.split()
        assert f[2] == str(i + 1) and [int(x) for x in f[4::2]] == w and f[3::2] == list(cm.FIELDS), line
    r = run("--clean", "1")
    assert r.returncode == 0 and r.stdout == cm.table_text(one), r.stderr
    r = run("--clean", "1", "--tip-keys", "0", "--island-keys", "0")
    assert r.returncode == 0 and r.stdout == cm.table_text(table), r.stderr
    r = run("--clean", "2", "--min-count", "2", "--histo", "10")
    f2 = cm.rounds(table, not forward, 2, 0, n_rounds=2)[0]
    hist = {}
    for c in f2.values():
        hist[min(c, 10)] = hist.get(min(c, 10), 0) + 1
    assert r.returncode == 0 and r.stdout == "".join("%d\t%d\n" % (c, hist[c]) for c in sorted(hist)), r.stderr


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("n_rows", [1023, 1024, 1025, 2049])
def test_view_rows_at_the_tile_seams(kmc, oracle, n_rows, canonical):
    """a view of exactly n_rows keys (a tile of the mark and scatter passes has 1024), kept and dropped rows mixed all over it"""
    k = 31
    rng = np.random.default_rng(7000 + n_rows)
    reads = ci.five_forks(k, 100 + k)[0] + [ci.rnd(rng, k + 2) for _ in range(40)]
    m = len(gm.count_table(reads, k, canonical))
    assert m < n_rows
    reads.append(ci.rnd(rng, n_rows - m + k - 1))                             # every window of it a new key
    kc, table = _counter(kmc, oracle, reads, k, canonical)
    assert len(table) == n_rows
    with kc:
        seen = _check(kmc, kc, table, canonical, ((1, 0),), ((k, k), (k, 0)))
    assert seen[((1, 0), (k, k))].summary[1:3] == [6, 40]


def _tool():
    import importlib.util
    spec = importlib.util.spec_from_file_location("measure_clean", os.path.join(ROOT, "tools", "measure_clean.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("canonical", [True, False])
def test_view_of_more_tiles_than_workgroups(kmc, canonical):
    """More than 2^21 rows: a workgroup of the mark pass walks several tiles, the tile counts fill more than one scan block.
    No Python model walks a table of this size; the expected answer is computed with numpy from the library's own unitigs,
    links and table (tools/measure_clean.host_clean, which test_clean_host.py checks against the model)."""
    k, n_reads = 31, 5800
    tool = _tool()
    sb, so = kmc.synth_reads_host(kmc.Synth(seed=77, pool=0), 0, n_reads)      # 400-base reads, every line fresh random
    rng = np.random.default_rng(77)
    tail = lambda n: rng.integers(0, 4, n).astype(np.uint8).view(np.uint8)
    code = np.frombuffer(b"ACGT", np.uint8)
    # off every fourth read a dead-end arm of 5 keys (a tip beside the rest of the read); 2000 reads of 3 keys (islands);
    # the first 500 reads twice (counts of 2)
    arms = [np.concatenate([sb[int(so[i]) + 100:int(so[i]) + 200], code[tail(5)]]) for i in range(0, n_reads, 4)]
    isl = [code[tail(k + 2)] for _ in range(2000)]
    extra = arms + isl + [sb[int(so[i]):int(so[i + 1])] for i in range(500)]
    bases = np.concatenate([sb] + extra)
    offs = np.concatenate([so, so[-1] + np.cumsum([len(x) for x in extra]).astype(U64)])
    with kmc.KmerCounter(k=k, canonical=canonical) as kc:
        kc.add_batch(bases, offs)
        table = kc.export()
        assert table.n_distinct > (1 << 21) + 4096
        u, lk = kc.unitigs(1, 0), kc.unitig_links(1, 0)
        for tip, isl_keys in ((k, k), (0, BIG)):
            lo, cnt, verdict, words = tool.host_clean(table, u, lk, k, canonical, tip, isl_keys)
            r = kc.clean_unitigs(1, 0, tip, isl_keys)
            assert r.summary.words() == words, (r.summary.words(), words)
            assert np.array_equal(r.verdict, verdict) and np.array_equal(r.table.key_lo, lo) and np.array_equal(r.table.count, cnt)
            assert not r.table.key_hi.any()
            if tip:
                assert words[1] >= 1400 and words[2] >= 1990 and words[0] > 8000, words
        dh, dl, dc, dv, nk, nu, s = kc.clean_unitigs_device(1, 0, k, k)
        lo, cnt, verdict, words = tool.host_clean(table, u, lk, k, canonical, k, k)
        assert s.words() == words and np.array_equal(_dev_u64(dl, nk), lo) and np.array_equal(_dev_u64(dc, nk), cnt)
        assert np.array_equal(_dev_bytes(dv, nu), verdict)


def test_cli_clean_with_queries_and_stats(kmc, tmp_path):
    """--query-kmers asks the cleaned table; the closing --stats line still describes the counting of the file"""
    k = 21
    reads = ci.rounds_input(k, 400 + k)
    fa = tmp_path / "rounds.fasta"
    fa.write_text("".join(">r%d\n%s\n" % (i, s) for i, s in enumerate(reads)))
    table = gm.count_table(reads, k, True)
    one = cm.rounds(table, True, n_rounds=1)[0]
    gone = sorted(set(table) - set(one))
    assert gone and one
    asked = gone[:3] + sorted(one)[:3]
    q = tmp_path / "kmers.txt"
    q.write_text("".join(x + "\n" for x in asked))
    r = subprocess.run([EXE, str(fa), "-k", str(k), "--clean", "1", "--query-kmers", str(q)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "".join("%s\t%d\n" % (x, one.get(x, 0)) for x in asked), r.stderr
    r = subprocess.run([EXE, str(fa), "-k", str(k), "--clean", "1", "--stats"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == cm.table_text(one), r.stderr
    last = [l for l in r.stderr.splitlines() if l.startswith("reads ")]
    assert len(last) == 1
    f = last[0].split()
    assert int(f[1]) == len(reads) and int(f[3]) == sum(len(s) for s in reads) and int(f[5]) == sum(table.values()), last
