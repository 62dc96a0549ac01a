"""GPU checks of kmc_unitig_components / kmc_unitig_components_device / kmc_unitig_components_into and
KmerCounter.components / components_device / components_into (kmc_components.hip.h).  Expected values come from
tests/components_model.py -- the definition of include/kmc.h as a union-find on the unitigs and links of unitig_model.py /
links_model.py -- applied to the CPU oracle's table of the same input.  All comparisons are exact: the component per unitig,
the four words per component, the verdicts, the kept table in view order and the eight summary words, through every form of
the call."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import clean_model as cm
import components_inputs as xi
import components_model as xm
import graph_model as gm
import links_model as lm
import unitig_model as um
from conftest import ROOT, SAMPLE
from test_clean_gpu import _counter
from test_unitig_gpu import _dev_bytes, _dev_u64, _table_dict

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "bin", "k-mer-count")
U64, U32, U8 = np.uint64, np.uint32, np.uint8
RANGES = ((1, 0), (2, 0), (1, 1), (2, 3))
BIG = 1 << 31
NAMES = ("comp_of", "stats", "verdict", "key_hi", "key_lo", "count")


def _limits(k):
    return (0, 1, k, BIG)


def _want(kmc, c):
    """(comp_of, stats, verdict, key_hi, key_lo, count) of a model result, the kept keys in view order"""
    keys = sorted(c.kept)
    enc = [kmc.encode_key(x, False) for x in keys]
    return (np.array(c.comp_of, U32), np.array(c.stats, U64).reshape(len(c.stats), 4), np.array(c.verdict, U8),
            np.array([e[0] for e in enc], U64), np.array([e[1] for e in enc], U64), np.array([c.kept[x] for x in keys], U64))


def _equal(got, want, ctx):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (ctx, name, g[:20], w[:20])


def _raw(kmc, kc, lo, hi, lim, nc, nu, nk, spare=3):
    """kmc_unitig_components through ctypes into arrays with `spare` entries more than needed, filled with a pattern"""
    L = kmc.lib()
    keys = [np.full(nk + spare, 0xEEEE, U64) for _ in range(3)]
    comp, ver = np.full(nu + spare, 0xEEEEEEEE, U32), np.full(nu + spare, 0xEE, U8)
    st = np.full((nc + spare) * 4, 0xEEEE, U64)
    n = [C.c_uint64(12345) for _ in range(3)]
    w = (C.c_uint64 * (kmc.COMPONENT_WORDS + 2))(*([0xEEEE] * 10))
    kc._chk(L.kmc_unitig_components(kc._h, lo, hi, lim, comp.ctypes.data, ver.ctypes.data, nu + spare, st.ctypes.data, nc + spare,
                                    keys[0].ctypes.data, keys[1].ctypes.data, keys[2].ctypes.data, nk + spare, *[C.byref(x) for x in n], w))
    assert [x.value for x in n] == [nc, nu, nk] and list(w)[8:] == [0xEEEE] * 2
    assert all((x[nk:] == 0xEEEE).all() for x in keys) and (comp[nu:] == 0xEEEEEEEE).all() and (ver[nu:] == 0xEE).all()
    assert (st[4 * nc:] == 0xEEEE).all()
    return (comp[:nu], st[:4 * nc].reshape(nc, 4), ver[:nu], keys[0][:nk], keys[1][:nk], keys[2][:nk]), list(w)[:8]


def _check(kmc, kc, table, canonical, ranges, limits, boundary=0):
    """every form of the call against the model, for every range and limit; with `boundary` also the limits at and one below
    the key counts of the smallest `boundary` distinct component sizes.  Returns {(range, limit): the model's result}"""
    L = kmc.lib()
    seen = {}
    for lo, hi in ranges:
        graph = (um.unitigs(table, canonical, lo, hi), lm.links(table, canonical, lo, hi))
        sizes = sorted({s[2] for s in xm.components(table, canonical, lo, hi, 0, graph=graph).stats})[:boundary]
        for lim in tuple(limits) + tuple(x for v in sizes for x in (v - 1, v) if x not in limits and x > 0):
            c = xm.components(table, canonical, lo, hi, lim, graph=graph)
            want, words = _want(kmc, c), c.summary
            nu, nc, nk = words[0], words[1], words[6]
            ctx = (kc.k, canonical, lo, hi, lim)
            # the identities of kmc.h, on the expected values
            assert nu == graph[0].summary[0] and sum(s[2] for s in c.stats) == graph[0].summary[2]
            assert sum(s[3] for s in c.stats) == graph[0].summary[7] and words[2] >= graph[1].summary[6]
            # the sizing call
            n = [C.c_uint64(1) for _ in range(3)]
            w = (C.c_uint64 * 8)()
            kc._chk(L.kmc_unitig_components(kc._h, lo, hi, lim, None, None, 0, None, 0, None, None, None, 0, *[C.byref(x) for x in n], w))
            assert ([x.value for x in n], list(w)) == ([nc, nu, nk], words), (ctx, list(w), words)
            got, w = _raw(kmc, kc, lo, hi, lim, nc, nu, nk)
            assert w == words, (ctx, w, words)
            _equal(got, want, ctx)
            # the device form, read back
            dco, dst, dv, dh, dl, dc, dnc, dnu, dnk, s = kc.components_device(lo, hi, lim)
            assert (dnc, dnu, dnk, s.words()) == (nc, nu, nk, words), (ctx, s.words(), words)
            assert dco and dst and dv and dl and dc and dst % 8 == 0 and dl % 8 == 0 and dc % 8 == 0 and bool(dh) == (kc.k > 31)
            g_hi = _dev_u64(dh, nk) if dh else np.zeros(nk, U64)
            _equal((_dev_bytes(dco, 4 * nu).view(U32), _dev_u64(dst, 4 * nc).reshape(nc, 4), _dev_bytes(dv, nu), g_hi, _dev_u64(dl, nk),
                    _dev_u64(dc, nk)), want, ctx)
            r = kc.components(lo, hi, lim)
            _equal((r.comp_of, r.stats, r.verdict, r.table.key_hi, r.table.key_lo, r.table.count), want, ctx)
            assert r.summary.words() == words and r.table.n_distinct == nk and r.to_text() == c.text()
            if nc:
                assert r.members(nc - 1).tolist() == c.members(nc - 1)
            if lim == 0:
                assert r.table.equals(kc.export_filtered(lo, hi)), ctx
            seen[((lo, hi), lim)] = c
        # the identities, on the library's own words
        t, l = kc.unitigs(lo, hi).summary.words(), kc.unitig_links(lo, hi).summary.words()
        r = kc.components(lo, hi)
        s = r.summary.words()
        assert int(r.stats[:, 1].sum()) == s[0] == t[0] and int(r.stats[:, 2].sum()) == t[2] and s[2] >= l[6]
        assert sum(int(x) for x in r.stats[:, 3]) == t[7]
    return seen


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [5, 15, 21, 31, 32, 33, 47, 63])
def test_sample_fasta(kmc, oracle, k, canonical):
    """(k = 32 canonical has the palindromic keys: records that are not symmetric)"""
    bases, offs = kmc.parse_fasta(SAMPLE)
    want = oracle.count_kmers(bases, offs, k, canonical)
    with kmc.KmerCounter(k=k, canonical=canonical) as kc:
        kc.add_batch(bases, offs)
        assert kc.export().equals(want)
        _check(kmc, kc, _table_dict(want), canonical, RANGES, _limits(k))


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [5, 31, 32, 63])
def test_built_inputs(kmc, oracle, k, canonical):
    """the ladder of 40 bubbles (many label rounds), 300 islands beside a fork (a second workgroup, waves of mixed
    components), the comb (waves of one component), components of n and n + 1 keys, a circular read, a hairpin, two forks,
    every bubble shape, the input of the rounds test -- with the limits at their boundaries"""
    seen = {}
    for name, reads in xi.built(k).items():
        kc, table = _counter(kmc, oracle, reads, k, canonical)
        with kc:
            seen[name] = _check(kmc, kc, table, canonical, ((1, 0),), _limits(k), boundary=3)
    if k < 31:
        return
    assert seen["ladder"][((1, 0), 0)].summary[:2] == [121, 1] and seen["comb"][((1, 0), 0)].summary[:2] == [141, 1]
    assert seen["islands_and_fork"][((1, 0), 0)].summary[:3] == [303, 301, 300]
    assert seen["boundary"][((1, 0), k + 3)].summary[5] == 1 and seen["boundary"][((1, 0), k + 2)].summary[5] == 0
    c = seen["circular"][((1, 0), BIG)]
    assert sum(c.unitigs.flags) == 1 and all(v == xm.COMPONENT for v in c.verdict) and c.summary[6] == 0


def test_empty_view_and_nothing_solid(kmc):
    bases, offs = kmc.parse_fasta(SAMPLE)
    with kmc.KmerCounter(k=31) as kc:
        kc.add_batch(bases, offs)
        kc.finalize()
        for lim in (0, 31, BIG):
            r = kc.components(10 ** 9, 0, lim)
            assert r.summary.words() == [0] * 8 and r.comp_of.shape == (0,) and r.stats.shape == (0, 4) and r.table.n_distinct == 0
            d = kc.components_device(10 ** 9, 0, lim)
            assert d[6:9] == (0, 0, 0) and d[9].words() == [0] * 8 and d[0] and d[1] and d[2] and d[4] and d[5]
        kc.reset()
        kc.finalize()
        r = kc.components()
        assert r.summary.words() == [0] * 8 and r.verdict.shape == (0,) and r.to_text() == ""
        with kmc.KmerCounter(k=31) as dst:
            assert kc.components_into(dst, 1, 0, 31).words() == [0] * 8 and dst.finalize() == (0, 0)


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [21, 32, 33])
def test_components_into_and_a_second_round(kmc, oracle, k, canonical):
    reads = xi.built(k)["rounds_input"] + xi.built(k)["boundary"] + xi.built(k)["two_forks"]
    kc, table = _counter(kmc, oracle, reads, k, canonical)
    with kc:
        digest = kc.export().digest()
        for lo, hi, lim in ((1, 0, k + 3), (2, 0, k + 3), (1, 0, 0), (1, 0, BIG)):
            final, words = xm.rounds(table, canonical, lo, hi, lim, n_rounds=2)
            with kmc.KmerCounter(k=k, canonical=canonical) as dst:
                s = kc.components_into(dst, lo, hi, lim)
                assert s.words() == words[0]
                dst.finalize()
                first = xm.components(table, canonical, lo, hi, lim).kept
                assert _table_dict(dst.export()) == first if first else dst.export().n_distinct == 0
                # the same limit again removes nothing more
                with kmc.KmerCounter(k=k, canonical=canonical) as dst2:
                    s2 = dst.components_into(dst2, lo, hi, lim)
                    dst2.finalize()
                    if first:
                        assert s2.words() == xm.components(first, canonical, lo, hi, lim).summary and s2.small == 0
                        assert _table_dict(dst2.export()) == first == final
                    else:
                        assert s2.words() == [0] * 8
        assert kc.export().digest() == digest               # the source is as it was
        # two sources into one dst: the counts of the keys both keep add up
        with kmc.KmerCounter(k=k, canonical=canonical) as dst:
            kc.components_into(dst, 1, 0, k + 3)
            kc.components_into(dst, 1, 0, k + 3)
            dst.finalize()
            first = xm.components(table, canonical, limit=k + 3).kept
            assert _table_dict(dst.export()) == {x: 2 * n for x, n in first.items()}


_CHILD = r"""
import importlib, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
kmc = importlib.import_module("k-mer-count_amd")
bases, offs = kmc.parse_fasta(sys.argv[2])
with kmc.KmerCounter(k=31) as kc, kmc.KmerCounter(k=31) as dst:
    kc.add_batch(bases, offs)
    kc.finalize()
    step = lambda s: print("step " + s, file=sys.stderr, flush=True)
    step("links(1,0)")
    kc.unitig_links(1, 0)
    step("components(1,0)")
    a = kc.components(1, 0)
    step("components(1,0) again")
    b = kc.components(1, 0)
    assert a.table.equals(b.table) and np.array_equal(a.comp_of, b.comp_of)
    step("components(1,0) other limit")
    kc.components(1, 0, 31)
    step("clean and simplify in between")
    kc.clean_unitigs(1, 0)
    kc.simplify_unitigs(1, 0)
    kc.components(1, 0, 31)
    step("components_device(1,0)")
    kc.components_device(1, 0, 31)
    step("components_into(1,0)")
    kc.components_into(dst, 1, 0, 31)
    step("links_device(1,0) components(1,0)")
    kc.unitig_links_device(1, 0)
    kc.components(1, 0, 31)
    step("graph(2,0) components(1,0)")
    kc.graph(2, 0, adj=False)
    kc.components(1, 0, 31)                 # (its own result is still there: nothing runs)
    kc.components_device(1, 0, 31)
    step("components(2,0)")
    kc.components(2, 0)
    step("unitigs(3,0) components(3,0)")
    kc.unitigs_device(3, 0)
    kc.components(3, 0)
    step("finalize components(2,0)")
    kc.add_batch(bases, offs)
    kc.finalize()
    kc.components(2, 0)
    step("end")
print("mem", *kmc.debug_mem())
"""


def test_components_reuse_the_held_unitigs_and_links_and_free_everything(kmc):
    """What computes, seen through the KMC_UNITIG_TRACE lines of a fresh child process (nothing is timed), and what the
    allocator's counters say when both contexts are closed"""
    env = dict(os.environ, KMC_UNITIG_TRACE="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, SAMPLE], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    steps, cur = {}, None
    fields = ["keys", "unitigs", "records", "components", "small", "kept", "rounds", "label_ms", "number_ms", "stats_ms", "keep_ms"]
    for line in r.stderr.splitlines():
        if line.startswith("step "):
            cur = line[5:]
            steps[cur] = []
        elif line.split(":")[0] in ("kmc_unitigs", "kmc_unitig_links", "kmc_unitig_clean", "kmc_unitig_simplify", "kmc_unitig_components"):
            steps[cur].append(line.split(":")[0])
            if line.startswith("kmc_unitig_components:"):
                assert line.split()[1::2] == fields and int(line.split()[14]) >= 1, line
            if line.startswith("kmc_unitig_links:"):
                steps[cur].append("unitigs_reused " + line.split("unitigs_reused ")[1].split()[0])
    x = "kmc_unitig_components"
    assert steps["links(1,0)"] == ["kmc_unitigs", "kmc_unitig_links", "unitigs_reused 0"]
    # behind the links of the same range: neither a unitigs nor a links line, and sizing then copy is one pass
    assert steps["components(1,0)"] == [x]
    assert steps["components(1,0) again"] == []
    assert steps["components(1,0) other limit"] == [x]                       # the limit is part of the key of the held result
    # a clean or a simplify result is another result: neither ends this one
    assert steps["clean and simplify in between"] == ["kmc_unitig_clean", "kmc_unitig_simplify"]
    assert steps["components_device(1,0)"] == [x] and steps["components_into(1,0)"] == [x]       # the device form always runs the pass
    # whatever drops the links drops the result: the links run again on the held unitigs, then the pass
    assert steps["links_device(1,0) components(1,0)"] == ["kmc_unitig_links", "unitigs_reused 1", x]
    # a graph call has rewritten adj: everything is computed again
    assert steps["graph(2,0) components(1,0)"] == ["kmc_unitigs", "kmc_unitig_links", "unitigs_reused 0", x]
    assert steps["components(2,0)"] == ["kmc_unitigs", "kmc_unitig_links", "unitigs_reused 0", x]
    # behind the unitigs of the range alone: the links pass runs on them, the unitigs do not run again
    assert steps["unitigs(3,0) components(3,0)"] == ["kmc_unitigs", "kmc_unitig_links", "unitigs_reused 1", x]
    assert steps["finalize components(2,0)"] == ["kmc_unitigs", "kmc_unitig_links", "unitigs_reused 0", x]  # a new view
    mem = [int(v) for v in r.stdout.split("mem")[1].split()]
    assert mem[0] == 0 and mem[1] == 0 and mem[4] == 0 and mem[2] > 0, mem     # live device / pinned bytes, failed frees


def test_nothing_else_moved(kmc, oracle):
    """the arrays a preceding unitigs, links or simplify call handed out are byte-identical after the components calls"""
    bases, offs = kmc.parse_fasta(SAMPLE)
    for k in (31, 63):
        want = oracle.count_kmers(bases, offs, k, True)
        table = _table_dict(want)
        with kmc.KmerCounter(k=k) as kc:
            kc.add_batch(bases, offs)
            kc.finalize()
            digest = kc.export().digest()
            vp = kc.export_device()
            db, do, da, df, nu, nb, _ = kc.unitigs_device(2, 0)
            lo_, lt, lnu, nl, _ = kc.unitig_links_device(2, 0)
            sh, sl, sc, sv, snk, snu, ss = kc.simplify_unitigs_device(2, 0)
            assert snu == nu == lnu
            arrays = ((do, 8 * (nu + 1)), (da, 8 * nu), (lo_, 8 * (2 * nu + 1)), (db, nb), (df, nu), (lt, 4 * nl), (sl, 8 * snk), (sc, 8 * snk),
                      (sv, nu)) + (((sh, 8 * snk),) if sh else ())
            read = lambda: [_dev_bytes(ptr, m) for ptr, m in arrays]
            before = read()
            _check(kmc, kc, table, True, ((2, 0),), (k, 0))     # on the unitigs and links the ctx holds
            after = read()
            assert all(np.array_equal(a, b) for a, b in zip(before, after))
            assert kc.simplify_unitigs(2, 0).summary.words() == ss.words()
            assert kc.export_device() == vp and kc.export().digest() == digest


def test_state_and_errors(kmc, oracle):
    L = kmc.lib()
    bases, offs = kmc.parse_fasta(SAMPLE)
    table = _table_dict(oracle.count_kmers(bases, offs, 31, True))
    n = [C.c_uint64(99) for _ in range(3)]
    nref = [C.byref(x) for x in n]
    w = (C.c_uint64 * 8)(*([7] * 8))
    p = [C.c_void_p(1) for _ in range(6)]

    def host(kc, lo, hi):
        return L.kmc_unitig_components(kc._h, lo, hi, 31, None, None, 0, None, 0, None, None, None, 0, *nref, w)

    def device(kc, lo, hi):
        return L.kmc_unitig_components_device(kc._h, lo, hi, 31, *[C.byref(x) for x in p], *nref, w)

    assert L.kmc_unitig_components(None, 1, 0, 31, None, None, 0, None, 0, None, None, None, 0, None, None, None, None) == kmc.ERR_ARG
    with kmc.KmerCounter(k=31) as kc, kmc.KmerCounter(k=31) as dst:
        assert host(kc, 1, 0) == kmc.ERR_STATE and device(kc, 1, 0) == kmc.ERR_STATE          # no view: before any finalize
        assert L.kmc_unitig_components_into(kc._h, dst._h, 1, 0, 31, None) == kmc.ERR_STATE
        kc.add_batch(bases, offs)
        assert host(kc, 1, 0) == kmc.ERR_STATE and device(kc, 1, 0) == kmc.ERR_STATE
        kc.finalize()
        # every output pointer may be NULL
        assert L.kmc_unitig_components_device(kc._h, 1, 0, 31, *([None] * 10)) == kmc.OK
        assert L.kmc_unitig_components(kc._h, 1, 0, 31, None, None, 0, None, 0, None, None, None, 0, None, None, None, None) == kmc.OK
        # max below min
        assert host(kc, 3, 2) == kmc.ERR_ARG and device(kc, 3, 2) == kmc.ERR_ARG
        assert L.kmc_unitig_components_into(kc._h, dst._h, 3, 2, 31, None) == kmc.ERR_ARG
        assert host(kc, 3, 3) == kmc.OK
        c = xm.components(table, True, limit=31)
        nu, nc, nk = c.summary[0], c.summary[1], c.summary[6]
        assert host(kc, 1, 0) == kmc.OK and ([x.value for x in n], list(w)) == ([nc, nu, nk], c.summary)
        # caps one too small: the sizes are set, nothing is copied
        a = [np.full(nk, 0xEEEE, U64) for _ in range(3)]
        comp, v, st = np.full(nu, 0xEEEEEEEE, U32), np.full(nu, 0xEE, U8), np.full(4 * nc, 0xEEEE, U64)
        for cu, cc, ck in ((nu - 1, nc, nk), (nu, nc - 1, nk), (nu, nc, nk - 1), (0, 0, 0)):
            for x in n:
                x.value = 0
            assert L.kmc_unitig_components(kc._h, 1, 0, 31, comp.ctypes.data, v.ctypes.data, cu, st.ctypes.data, cc, a[0].ctypes.data, a[1].ctypes.data,
                                           a[2].ctypes.data, ck, *nref, w) == kmc.ERR_ARG
            assert [x.value for x in n] == [nc, nu, nk] and b"kmc_unitig_components" in L.kmc_last_error(kc._h)
            assert all((x == 0xEEEE).all() for x in a) and (v == 0xEE).all() and (comp == 0xEEEEEEEE).all() and (st == 0xEEEE).all()
        # an array that is NULL has no cap
        assert L.kmc_unitig_components(kc._h, 1, 0, 31, None, v.ctypes.data, nu, None, 0, None, None, None, 0, None, None, None, None) == kmc.OK
        assert np.array_equal(v, np.array(c.verdict, U8)) and all((x == 0xEEEE).all() for x in a) and (st == 0xEEEE).all()
        # kmc_unitig_components_into: dst must be another ctx of the same kind
        assert L.kmc_unitig_components_into(kc._h, kc._h, 1, 0, 31, None) == kmc.ERR_ARG
        assert L.kmc_unitig_components_into(kc._h, None, 1, 0, 31, None) == kmc.ERR_ARG
        assert L.kmc_unitig_components_into(None, dst._h, 1, 0, 31, None) == kmc.ERR_ARG
        for kw in (dict(k=33), dict(k=31, canonical=False)):
            with kmc.KmerCounter(**kw) as bad:
                assert L.kmc_unitig_components_into(kc._h, bad._h, 1, 0, 31, None) == kmc.ERR_ARG
                assert b"differ in" in L.kmc_last_error(kc._h)
                with pytest.raises(kmc.KmcError) as e:
                    kc.components_into(bad)
                assert e.value.status == kmc.ERR_ARG
        assert dst.finalize() == (0, 0)                      # nothing reached dst through the failed calls
        kc.reset()
        assert host(kc, 1, 0) == kmc.ERR_STATE and device(kc, 1, 0) == kmc.ERR_STATE
    with kmc.KmerCounter(mode=kmc.MODE_LR) as kc, kmc.KmerCounter(mode=kmc.MODE_LR) as dst:
        kc.count_file(SAMPLE)
        kc.finalize()
        assert host(kc, 1, 0) == kmc.ERR_ARG and device(kc, 1, 0) == kmc.ERR_ARG
        assert L.kmc_unitig_components_into(kc._h, dst._h, 1, 0, 31, None) == kmc.ERR_ARG
        with pytest.raises(kmc.KmcError) as e:
            kc.components()
        assert e.value.status == kmc.ERR_ARG


@pytest.mark.parametrize("forward", [False, True])
def test_cli_components_and_component_keys(kmc, tmp_path, forward):
    k = 21
    canonical = not forward
    reads = xi.built(k)["rounds_input"] + xi.built(k)["boundary"] + xi.built(k)["two_forks"]
    fa = tmp_path / "components.fasta"
    fa.write_text("".join(">r%d\n%s\n" % (i, s) for i, s in enumerate(reads)))
    table = gm.count_table(reads, k, canonical)
    fw = ["--forward"] if forward else []
    run = lambda *a: subprocess.run([EXE, str(fa), "-k", str(k)] + list(a) + fw, capture_output=True, text=True)
    r = run("--components")
    assert r.returncode == 0 and r.stdout == xm.components(table, canonical).text(), r.stderr
    r = run("--components", "--min-count", "2")
    assert r.returncode == 0 and r.stdout == xm.components(table, canonical, 2, 0).text(), r.stderr
    lim = k + 3
    c = xm.components(table, canonical, limit=lim)
    assert 0 < c.summary[5] < c.summary[1]
    r = run("--component-keys", str(lim), "--stats")
    assert r.returncode == 0 and r.stdout == cm.table_text(c.kept), r.stderr
    line = [l for l in r.stderr.splitlines() if l.startswith("component step ")]
    assert len(line) == 1 and [int(x) for x in line[0].split()[3::2]] == c.summary and line[0].split()[2::2] == list(xm.FIELDS), line
    r = run("--component-keys", str(lim), "--components")
    assert r.returncode == 0 and r.stdout == xm.components(c.kept, canonical).text(), r.stderr
    r = run("--component-keys", str(lim), "--gfa")
    assert r.returncode == 0 and r.stdout == lm.gfa(um.unitigs(c.kept, canonical), lm.links(c.kept, canonical), k), r.stderr
    r = run("--component-keys", "0")
    assert r.returncode == 0 and r.stdout == cm.table_text(table), r.stderr
    # behind the clean rounds
    cleaned = cm.rounds(table, canonical, n_rounds=3)[0]
    r = run("--clean", "3", "--component-keys", str(lim), "--unitigs")
    assert r.returncode == 0 and r.stdout == um.unitigs(xm.components(cleaned, canonical, limit=lim).kept, canonical).fasta(), r.stderr
