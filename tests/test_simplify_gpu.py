"""GPU checks of kmc_unitig_simplify / kmc_unitig_simplify_device / kmc_unitig_simplify_into and KmerCounter.simplify_unitigs /
simplified (kmc_clean.hip.h with BUBBLES).  Expected values come from tests/bubble_model.py -- the definition of
include/kmc.h on the unitigs and links of unitig_model.py / links_model.py -- applied to the CPU oracle's table of the same
input.  All comparisons are exact: the verdicts, the kept table in view order and the twelve summary words, through every
form of the call."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import bubble_inputs as bi
import bubble_model as bm
import clean_inputs as ci
import clean_model as cm
import graph_model as gm
import links_model as lm
import unitig_model as um
from conftest import ROOT, SAMPLE
from test_clean_gpu import _counter, _equal, _merged, _want
from test_links_gpu import _branching, _dev_u32
from test_unitig_gpu import _dev_bytes, _dev_u64, _same, _table_dict, _want_arrays

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "bin", "k-mer-count")
U64, U8 = np.uint64, np.uint8
RANGES = ((1, 0), (2, 0), (1, 1), (2, 3))
BIG = 1 << 31


def _limits(k):
    return ((k, k, k), (0, 0, 0), (0, 0, k), (k, k, 0), (BIG, BIG, BIG), (1, 1, 1))


def _raw(kmc, kc, lo, hi, lim, nk, nu, spare=3):
    """kmc_unitig_simplify through ctypes into arrays with `spare` entries more than needed, filled with a pattern"""
    L = kmc.lib()
    a = [np.full(nk + spare, 0xEEEE, U64) for _ in range(3)]
    v = np.full(nu + spare, 0xEE, U8)
    n1, n2 = C.c_uint64(12345), C.c_uint64(12345)
    w = (C.c_uint64 * (kmc.SIMPLIFY_WORDS + 2))(*([0xEEEE] * 14))
    kc._chk(L.kmc_unitig_simplify(kc._h, lo, hi, *lim, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, nk + spare, v.ctypes.data, nu + spare,
                                  C.byref(n1), C.byref(n2), w))
    assert (n1.value, n2.value) == (nk, nu) and list(w)[12:] == [0xEEEE] * 2
    assert all((x[nk:] == 0xEEEE).all() for x in a) and (v[nu:] == 0xEE).all()
    return (a[0][:nk], a[1][:nk], a[2][:nk], v[:nu]), list(w)[:12]


def _check(kmc, kc, table, canonical, ranges, limits):
    """every form of the call against the model, for every range and triple of limits; returns {(range, limits): the model's result}"""
    L = kmc.lib()
    seen = {}
    for lo, hi in ranges:
        graph = (um.unitigs(table, canonical, lo, hi), lm.links(table, canonical, lo, hi))
        for lim in limits:
            c = bm.simplify(table, canonical, lo, hi, *lim, graph=graph)
            want, words = _want(kmc, c), c.summary
            nk, nu = words[3], words[0]
            ctx = (kc.k, canonical, lo, hi, lim)
            assert words[3] + words[4] + words[5] + words[9] == graph[0].summary[2]
            # the sizing call
            n1, n2 = C.c_uint64(1), C.c_uint64(1)
            w = (C.c_uint64 * 12)()
            kc._chk(L.kmc_unitig_simplify(kc._h, lo, hi, *lim, None, None, None, 0, None, 0, C.byref(n1), C.byref(n2), w))
            assert (n1.value, n2.value, list(w)) == (nk, nu, words), (ctx, list(w), words)
            got, w = _raw(kmc, kc, lo, hi, lim, nk, nu)
            assert w == words, (ctx, w, words)
            _equal(got, want, ctx)
            # the device form, read back
            dh, dl, dc, dv, dnk, dnu, s = kc.simplify_unitigs_device(lo, hi, *lim)
            assert (dnk, dnu, s.words()) == (nk, nu, words), (ctx, s.words(), words)
            assert dl and dc and dv and dl % 8 == 0 and dc % 8 == 0 and bool(dh) == (kc.k > 31)
            g_hi = _dev_u64(dh, nk) if dh else np.zeros(nk, U64)
            _equal((g_hi, _dev_u64(dl, nk), _dev_u64(dc, nk), _dev_bytes(dv, nu)), want, ctx)
            r = kc.simplify_unitigs(lo, hi, *lim)
            _equal((r.table.key_hi, r.table.key_lo, r.table.count, r.verdict), want, ctx)
            assert r.summary.words() == words and r.table.n_distinct == nk
            if lim[2] == 0:
                # equivalence to clean: tables, verdicts and words [0..7] are kmc_unitig_clean's, [8..11] are 0
                old = kc.clean_unitigs(lo, hi, lim[0], lim[1])
                _equal((old.table.key_hi, old.table.key_lo, old.table.count, old.verdict), want, ctx)
                assert old.summary.words() == words[:8] and words[8:] == [0] * 4, ctx
            seen[((lo, hi), lim)] = c
        t = kc.unitigs(lo, hi).summary.words()
        s = kc.simplify_unitigs(lo, hi).summary.words()
        assert s[3] + s[4] + s[5] + s[9] == t[2] and s[0] == t[0]
    return seen


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [5, 15, 21, 31, 32, 33, 47, 63])
def test_sample_fasta(kmc, oracle, k, canonical):
    bases, offs = kmc.parse_fasta(SAMPLE)
    want = oracle.count_kmers(bases, offs, k, canonical)
    with kmc.KmerCounter(k=k, canonical=canonical) as kc:
        kc.add_batch(bases, offs)
        assert kc.export().equals(want)
        _check(kmc, kc, _table_dict(want), canonical, RANGES, _limits(k))


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [5, 31, 32, 63])
def test_built_inputs(kmc, oracle, k, canonical):
    """the substitution bubble, three arms, arms of k and k + 1 keys, pairs decided at each level, a tip and a bubble at one
    junction, a circular read, a unitig whose two ends reach the same end -- one by one and all in one table"""
    inputs = {"substitution": bi.substitution(k, 10 + k)[0], "three_arms": bi.three_arms(k, 20 + k)[0],
              "k_and_k_plus_1": bi.arms_k_and_k_plus_1(k, 30 + k)[0], "decided_pairs": bi.decided_pairs(k, 40 + k)[0],
              "tip_and_bubble": bi.tip_and_bubble(k, 60 + k)[0], "circular": [bi.circular(k, 70 + k)] + bi.substitution(k, 10 + k)[0],
              "same_end": bi.same_end(k, 80 + k)[0], "everything": bi.everything(k, 90 + k)}
    seen = {}
    for name, reads in inputs.items():
        kc, table = _counter(kmc, oracle, reads, k, canonical)
        with kc:
            seen[name] = _check(kmc, kc, table, canonical, ((1, 0),), _limits(k) + ((k, k, k + 1),))
    if k < 21:
        return
    kk = ((1, 0), (k, k, k))
    assert seen["substitution"][kk].summary == [4, 0, 0, 5 * k + 1, 0, 0, 0, 3 * (5 * k + 1), 1, k, 2, k]
    assert seen["three_arms"][kk].summary[8:11] == [2, 2 * k, 3]
    assert seen["k_and_k_plus_1"][kk].summary[8:11] == [1, k, 2] and seen["k_and_k_plus_1"][((1, 0), (k, k, k + 1))].summary[8:11] == [2, 2 * k + 1, 4]
    assert seen["decided_pairs"][kk].bubble_levels == {"abundance": 2, "keys": 2, "id": 2} and seen["decided_pairs"][kk].summary[8] == 3
    assert seen["tip_and_bubble"][kk].summary[1] == 1 and seen["tip_and_bubble"][kk].summary[8] == 1
    assert seen["circular"][kk].summary[8] == 1 and sum(seen["circular"][kk].unitigs.flags) == 1
    assert seen["same_end"][((1, 0), (BIG, BIG, BIG))].summary[8] == 0


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [6, 21, 32, 33, 63])
def test_branching_reads(kmc, oracle, k, canonical):
    """hairpins, palindromes for even k, dropped records, circular unitigs (all kept), bubbles of the links test, limits 3k"""
    kc, table = _counter(kmc, oracle, _branching(k, 900 + k), k, canonical)
    with kc:
        seen = _check(kmc, kc, table, canonical, ((1, 0), (2, 0)), ((3 * k, 3 * k, 3 * k), (0, 0, BIG)))
    c = seen[((1, 0), (3 * k, 3 * k, 3 * k))]
    assert all(c.verdict[u] == bm.KEEP for u, f in enumerate(c.unitigs.flags) if f)
    if k >= 21:
        assert sum(c.unitigs.flags) > 0 and c.summary[8] >= 3, c.summary


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [5, 21, 32, 33, 63])
def test_wide_products(kmc, k, canonical):
    """mean abundances of two parallel arms whose comparison needs more than 64 bits of product"""
    table, true_arm, ins_arm = bi.wide_bubble(k, canonical, 50 + k)
    with _merged(kmc, table, k, canonical) as kc:
        seen = _check(kmc, kc, table, canonical, ((1, 0),), ((k, k, k),))
    c = seen[((1, 0), (k, k, k))]
    ut, ui = bi.unitig_with(c.unitigs, true_arm[0], k, canonical), bi.unitig_with(c.unitigs, ins_arm[0], k, canonical)
    assert (c.verdict[ut], c.verdict[ui]) == (bm.BUBBLE, bm.KEEP)
    assert c.summary[11] == ((1 << 64) - 1) // k


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("n_rows", [1023, 1024, 1025, 2049])
def test_view_rows_at_the_tile_seams(kmc, oracle, n_rows, canonical):
    """a view of exactly n_rows keys (a tile of the mark and scatter passes has 1024): kept, tip, island and bubble rows mixed"""
    k = 31
    rng = np.random.default_rng(8000 + n_rows)
    reads = ci.five_forks(k, 100 + k)[0] + [ci.rnd(rng, k + 2) for _ in range(20)]
    for i in range(3):
        reads += bi.substitution(k, 500 + i)[0]
    m = len(gm.count_table(reads, k, canonical))
    assert m < n_rows
    reads.append(ci.rnd(rng, n_rows - m + k - 1))                             # every window of it a new key
    kc, table = _counter(kmc, oracle, reads, k, canonical)
    assert len(table) == n_rows
    with kc:
        seen = _check(kmc, kc, table, canonical, ((1, 0),), ((k, k, k), (k, 0, k), (k, k, 0)))
    s = seen[((1, 0), (k, k, k))].summary
    assert s[1:3] == [6, 20 + (n_rows - m <= k)] and s[8:11] == [3, 3 * k, 6]       # (a short filler read is an island too)


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [5, 31, 32, 63])
def test_field_of_bubbles(kmc, oracle, k, canonical):
    """320 independent bubbles, 1280 unitigs: the verdict kernel runs five workgroups and every wave adds partial sums
    (at k = 5 the 320 sequences run into one another: whatever that graph is, the model walks it too)"""
    reads, errs = bi.field(k, 100 + k)
    kc, table = _counter(kmc, oracle, reads, k, canonical)
    with kc:
        seen = _check(kmc, kc, table, canonical, ((1, 0),), ((k, k, k), (0, 0, k)))
    for lim in ((k, k, k), (0, 0, k)) if k >= 31 else ():
        c = seen[((1, 0), lim)]
        assert c.summary[0] == 1280 and c.summary[8:] == [320, 320 * k, 640, 320 * k]
        popped = {u for u, v in enumerate(c.verdict) if v == bm.BUBBLE}
        assert popped == {bi.unitig_with(c.unitigs, e[:k], k, canonical) for e in errs[::16]} | popped and len(popped) == 320


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [21, 32, 33])
def test_simplify_into_and_simplified_rounds(kmc, oracle, k, canonical):
    reads = ci.rounds_input(k, 400 + k) + bi.substitution(k, 10 + k)[0] + bi.three_arms(k, 20 + k)[0]
    kc, table = _counter(kmc, oracle, reads, k, canonical)
    with kc:
        digest = kc.export().digest()
        for lo, hi in ((1, 0), (2, 0)):
            final, words = bm.rounds(table, canonical, lo, hi, n_rounds=4)
            out, got = kc.simplified(lo, hi, rounds=4)
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
                assert words[0][8] == 3 and sorted(len(s) - k + 1 for s in u.seqs) == sorted([5 * k + 1, k + 6, 5 * k + 1, 5 * k + 1])
        # the limits reach the library: bubble limit 0 is cleaned()
        out, got = kc.simplified(max_bubble_keys=0, rounds=4)
        with out:
            assert [s.words()[:8] for s in got] == cm.rounds(table, canonical, n_rounds=4)[1] and all(s.words()[8:] == [0] * 4 for s in got)
            assert _table_dict(out.export()) == cm.rounds(table, canonical, n_rounds=4)[0]
        assert kc.export().digest() == digest               # the source is as it was
    # the substitution input alone ends as one unitig
    kc, table = _counter(kmc, oracle, bi.substitution(k, 10 + k)[0], k, canonical)
    with kc:
        out, got = kc.simplified(rounds=4)
        with out:
            assert [s.words() for s in got] == bm.rounds(table, canonical, n_rounds=4)[1] and len(got) == 2
            r = out.unitigs()
            assert r.summary.words()[0] == 1 and len(r.bases) == 6 * k
        # two sources into one dst: the counts of the keys both keep add up
        other = bi.substitution(k, 10 + k)[0][:3] + bi.tip_and_bubble(k, 60 + k)[0]
        kc2, table2 = _counter(kmc, oracle, other, k, canonical)
        with kc2, kmc.KmerCounter(k=k, canonical=canonical) as dst:
            s1, s2 = kc.simplify_into(dst), kc2.simplify_into(dst)
            c1, c2 = bm.simplify(table, canonical), bm.simplify(table2, canonical)
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
    step = lambda s: print("step " + s, file=sys.stderr, flush=True)
    step("links(1,0)")
    kc.unitig_links(1, 0)
    step("simplify(1,0)")
    a = kc.simplify_unitigs(1, 0)
    step("simplify(1,0) again")
    b = kc.simplify_unitigs(1, 0)
    assert a.table.equals(b.table)
    step("clean(1,0) behind simplify")
    kc.clean_unitigs(1, 0)
    step("simplify(1,0) behind clean")
    kc.simplify_unitigs(1, 0)
    step("simplify(1,0) other bubble limit")
    kc.simplify_unitigs(1, 0, 31, 31, 5)
    step("simplify limit 0 then clean")
    kc.simplify_unitigs(1, 0, 31, 31, 0)
    kc.clean_unitigs(1, 0, 31, 31)
    step("simplify_device(1,0)")
    kc.simplify_unitigs_device(1, 0)
    step("graph(2,0) simplify(1,0)")
    kc.graph(2, 0, adj=False)
    kc.simplify_unitigs_device(1, 0)
    step("simplify(2,0)")
    kc.simplify_unitigs(2, 0)
    step("end")
"""


def test_simplify_reuses_the_held_unitigs_and_links(kmc):
    """What computes, seen through the KMC_UNITIG_TRACE lines of a child process (nothing is timed)"""
    env = dict(os.environ, KMC_UNITIG_TRACE="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, SAMPLE], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    steps, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("step "):
            cur = line[5:]
            steps[cur] = []
        elif line.split(":")[0] in ("kmc_unitigs", "kmc_unitig_links", "kmc_unitig_clean", "kmc_unitig_simplify"):
            steps[cur].append(line.split(":")[0])
            if line.startswith("kmc_unitig_simplify:"):
                assert [x for x in line.split()[1::2]] == ["keys", "unitigs", "tips", "islands", "bubbles", "kept", "clean_ms"], line
    assert steps["links(1,0)"] == ["kmc_unitigs", "kmc_unitig_links"]
    # behind the links of the same range: neither a unitigs nor a links line, and sizing then copy is one pass
    assert steps["simplify(1,0)"] == ["kmc_unitig_simplify"]
    assert steps["simplify(1,0) again"] == []
    # the bubble limit is part of the key of the held result, a clean call having limit 0
    assert steps["clean(1,0) behind simplify"] == ["kmc_unitig_clean"]
    assert steps["simplify(1,0) behind clean"] == ["kmc_unitig_simplify"]
    assert steps["simplify(1,0) other bubble limit"] == ["kmc_unitig_simplify"]
    assert steps["simplify limit 0 then clean"] == ["kmc_unitig_simplify"]
    # the device form always runs the pass
    assert steps["simplify_device(1,0)"] == ["kmc_unitig_simplify"]
    # a graph call has rewritten adj: both are computed again
    assert steps["graph(2,0) simplify(1,0)"] == ["kmc_unitigs", "kmc_unitig_links", "kmc_unitig_simplify"]
    assert steps["simplify(2,0)"] == ["kmc_unitigs", "kmc_unitig_links", "kmc_unitig_simplify"]


def test_nothing_else_moved(kmc, oracle):
    """the arrays a preceding unitigs or links call handed out are unchanged by the simplify calls behind them"""
    bases, offs = kmc.parse_fasta(SAMPLE)
    for k in (31, 63):
        want = oracle.count_kmers(bases, offs, k, True)
        table = _table_dict(want)
        with kmc.KmerCounter(k=k) as kc:
            kc.add_batch(bases, offs)
            kc.finalize()
            digest = kc.export().digest()
            vp = kc.export_device()
            fhi, flo, fcnt, nk, _ = kc.filter_device(2, 0)
            db, do, da, df, nu, nb, _ = kc.unitigs_device(2, 0)
            lo_, lt, lnu, nl, _ = kc.unitig_links_device(2, 0)
            arrays = ((flo, nk), (fcnt, nk), (do, nu + 1), (da, nu), (lo_, 2 * nu + 1))
            read = lambda: [_dev_u64(ptr, m) for ptr, m in arrays] + [_dev_bytes(db, nb), _dev_bytes(df, nu), _dev_u32(lt, nl)]
            before = read()
            _check(kmc, kc, table, True, ((2, 0),), ((k, k, k), (0, 0, 0)))     # on the unitigs and links the ctx holds
            after = read()
            assert all(np.array_equal(a, b) for a, b in zip(before, after))
            u, lk = um.unitigs(table, True, 2, 0), lm.links(table, True, 2, 0)
            _same((after[5], after[2], after[3], after[6]), _want_arrays(u), k)
            assert np.array_equal(after[4], np.array(lk.offsets, U64)) and np.array_equal(after[7], np.array(lk.to, np.uint32))
            assert kc.export_device() == vp and kc.export().digest() == digest


def test_state_and_errors(kmc, oracle):
    L = kmc.lib()
    bases, offs = kmc.parse_fasta(SAMPLE)
    table = _table_dict(oracle.count_kmers(bases, offs, 31, True))
    n1, n2 = C.c_uint64(99), C.c_uint64(99)
    w = (C.c_uint64 * 12)(*([7] * 12))
    p = [C.c_void_p(1) for _ in range(4)]

    def host(kc, lo, hi):
        return L.kmc_unitig_simplify(kc._h, lo, hi, 31, 31, 31, None, None, None, 0, None, 0, C.byref(n1), C.byref(n2), w)

    def device(kc, lo, hi):
        return L.kmc_unitig_simplify_device(kc._h, lo, hi, 31, 31, 31, *[C.byref(x) for x in p], C.byref(n1), C.byref(n2), w)

    assert L.kmc_unitig_simplify(None, 1, 0, 31, 31, 31, None, None, None, 0, None, 0, None, None, None) == kmc.ERR_ARG
    with kmc.KmerCounter(k=31) as kc, kmc.KmerCounter(k=31) as dst:
        assert host(kc, 1, 0) == kmc.ERR_STATE and device(kc, 1, 0) == kmc.ERR_STATE          # no view: before any finalize
        assert L.kmc_unitig_simplify_into(kc._h, dst._h, 1, 0, 31, 31, 31, None) == kmc.ERR_STATE
        kc.add_batch(bases, offs)
        assert host(kc, 1, 0) == kmc.ERR_STATE and device(kc, 1, 0) == kmc.ERR_STATE
        kc.finalize()
        # every output pointer may be NULL
        assert L.kmc_unitig_simplify_device(kc._h, 1, 0, 31, 31, 31, None, None, None, None, None, None, None) == kmc.OK
        assert L.kmc_unitig_simplify(kc._h, 1, 0, 31, 31, 31, None, None, None, 0, None, 0, None, None, None) == kmc.OK
        # max below min
        assert host(kc, 3, 2) == kmc.ERR_ARG and device(kc, 3, 2) == kmc.ERR_ARG
        assert L.kmc_unitig_simplify_into(kc._h, dst._h, 3, 2, 31, 31, 31, None) == kmc.ERR_ARG
        assert host(kc, 3, 3) == kmc.OK
        c = bm.simplify(table, True)
        nk, nu = c.summary[3], c.summary[0]
        assert host(kc, 1, 0) == kmc.OK and (n1.value, n2.value, list(w)) == (nk, nu, c.summary)
        # nothing solid
        assert host(kc, 10 ** 9, 0) == kmc.OK and (n1.value, n2.value, list(w)) == (0, 0, [0] * 12)
        d = kc.simplify_unitigs_device(10 ** 9, 0)
        assert d[4:6] == (0, 0) and d[6].words() == [0] * 12 and d[1] and d[2] and d[3]
        # caps one too small: the sizes are set, nothing is copied
        a = [np.full(nk, 0xEEEE, U64) for _ in range(3)]
        v = np.full(nu, 0xEE, U8)
        for ck, cu in ((nk - 1, nu), (nk, nu - 1), (0, 0)):
            n1.value = n2.value = 0
            assert L.kmc_unitig_simplify(kc._h, 1, 0, 31, 31, 31, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, ck, v.ctypes.data, cu,
                                         C.byref(n1), C.byref(n2), w) == kmc.ERR_ARG
            assert (n1.value, n2.value) == (nk, nu) and b"kmc_unitig_simplify" in L.kmc_last_error(kc._h)
            assert all((x == 0xEEEE).all() for x in a) and (v == 0xEE).all()
        assert L.kmc_unitig_simplify(kc._h, 1, 0, 31, 31, 31, None, None, None, 0, v.ctypes.data, nu, None, None, None) == kmc.OK
        assert np.array_equal(v, np.array(c.verdict, U8)) and all((x == 0xEEEE).all() for x in a)
        # kmc_unitig_simplify_into: dst must be another ctx of the same kind
        assert L.kmc_unitig_simplify_into(kc._h, kc._h, 1, 0, 31, 31, 31, None) == kmc.ERR_ARG
        assert L.kmc_unitig_simplify_into(kc._h, None, 1, 0, 31, 31, 31, None) == kmc.ERR_ARG
        assert L.kmc_unitig_simplify_into(None, dst._h, 1, 0, 31, 31, 31, None) == kmc.ERR_ARG
        for kw in (dict(k=33), dict(k=31, canonical=False)):
            with kmc.KmerCounter(**kw) as bad:
                assert L.kmc_unitig_simplify_into(kc._h, bad._h, 1, 0, 31, 31, 31, None) == kmc.ERR_ARG
                assert b"differ in" in L.kmc_last_error(kc._h)
                with pytest.raises(kmc.KmcError) as e:
                    kc.simplify_into(bad)
                assert e.value.status == kmc.ERR_ARG
        assert dst.finalize() == (0, 0)                      # nothing reached dst through the failed calls
        # an empty view
        kc.reset()
        assert host(kc, 1, 0) == kmc.ERR_STATE and device(kc, 1, 0) == kmc.ERR_STATE
        kc.finalize()
        r = kc.simplify_unitigs()
        assert r.table.n_distinct == 0 and r.verdict.shape == (0,) and r.summary.words() == [0] * 12
        with kmc.KmerCounter(k=31) as dst2:
            assert kc.simplify_into(dst2).words() == [0] * 12 and dst2.finalize() == (0, 0)
    with kmc.KmerCounter(mode=kmc.MODE_LR) as kc, kmc.KmerCounter(mode=kmc.MODE_LR) as dst:
        kc.count_file(SAMPLE)
        kc.finalize()
        assert host(kc, 1, 0) == kmc.ERR_ARG and device(kc, 1, 0) == kmc.ERR_ARG
        assert L.kmc_unitig_simplify_into(kc._h, dst._h, 1, 0, 31, 31, 31, None) == kmc.ERR_ARG
        with pytest.raises(kmc.KmcError) as e:
            kc.simplify_unitigs()
        assert e.value.status == kmc.ERR_ARG


@pytest.mark.parametrize("forward", [False, True])
def test_cli_bubble_keys(kmc, tmp_path, forward):
    k = 21
    canonical = not forward
    reads = ci.rounds_input(k, 400 + k) + bi.substitution(k, 10 + k)[0] + bi.three_arms(k, 20 + k)[0]
    fa = tmp_path / "bubbles.fasta"
    fa.write_text("".join(">r%d\n%s\n" % (i, s) for i, s in enumerate(reads)))
    table = gm.count_table(reads, k, canonical)
    fw = ["--forward"] if forward else []
    run = lambda *a: subprocess.run([EXE, str(fa), "-k", str(k)] + list(a) + fw, capture_output=True, text=True)
    final, w3 = bm.rounds(table, canonical, n_rounds=3)
    plain, p3 = cm.rounds(table, canonical, n_rounds=3)
    assert final != plain and w3[0][8] == 3
    r = run("--clean", "3", "--bubble-keys", str(k))
    assert r.returncode == 0 and r.stdout == cm.table_text(final), r.stderr
    r = run("--clean", "3", "--bubble-keys", str(k), "--unitigs")
    assert r.returncode == 0 and r.stdout == um.unitigs(final, canonical).fasta(), r.stderr
    r = run("--clean", "3", "--bubble-keys", str(k), "--gfa", "--stats")
    assert r.returncode == 0 and r.stdout == lm.gfa(um.unitigs(final, canonical), lm.links(final, canonical), k), r.stderr
    lines = [l for l in r.stderr.splitlines() if l.startswith("clean round ")]
    assert len(lines) == len(w3) == 2
    for i, (line, w) in enumerate(zip(lines, w3)):
        f = line.split()
        assert f[2] == str(i + 1) and [int(x) for x in f[4::2]] == w[:11] and f[3::2] == list(bm.FIELDS[:11]), line
    r = run("--clean", "3", "--bubble-keys", str(k), "--histo", "10")
    hist = {}
    for c in final.values():
        hist[min(c, 10)] = hist.get(min(c, 10), 0) + 1
    assert r.returncode == 0 and r.stdout == "".join("%d\t%d\n" % (c, hist[c]) for c in sorted(hist)), r.stderr
    # --bubble-keys 0 and no --bubble-keys pop nothing; without the option the output is what --clean always printed
    r = run("--clean", "3", "--stats")
    assert r.returncode == 0 and r.stdout == cm.table_text(plain), r.stderr
    lines = [l for l in r.stderr.splitlines() if l.startswith("clean round ")]
    assert len(lines) == len(p3)
    for i, (line, w) in enumerate(zip(lines, p3)):
        f = line.split()
        assert f[2] == str(i + 1) and [int(x) for x in f[4::2]] == w and f[3::2] == list(cm.FIELDS), line
    r = run("--clean", "3", "--bubble-keys", "0")
    assert r.returncode == 0 and r.stdout == cm.table_text(plain), r.stderr
    r = run("--bubble-keys", str(k))
    assert r.returncode == 2 and r.stdout == "" and "need --clean ROUNDS" in r.stderr
