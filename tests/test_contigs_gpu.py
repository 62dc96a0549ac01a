"""GPU checks of kmc_unitig_contigs / kmc_unitig_contigs_device / KmerCounter.contigs (kmc_contigs.hip.h).  Expected values come
from tests/contig_model.py -- the definitions of include/kmc.h over Python lists, on top of transit_model's counts and
unitig_model's spellings -- applied to the CPU oracle's table of the same input.  All comparisons are exact, array by array,
through every form of the call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import contig_inputs as ci
import contig_model as cm
import graph_model as gm
import map_inputs as mi
import transit_inputs as ti
import transit_model as tm
import unitig_model as um
from conftest import ROOT
from test_map_gpu import _counter
from test_unitig_gpu import _dev_bytes, _dev_u64

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "bin", "k-mer-count")
U64, U32, U8 = np.uint64, np.uint32, np.uint8
NEVER = 1 << 63
NAMES = ("bases", "offsets", "path_offsets", "path", "abund", "flags")
RANGES = ((1, 0), (2, 0))
MIN_READS = (1, ti.PAIR_DEPTH, ti.PAIR_DEPTH + 1)
MIN_SUPPORT = (0, 1, NEVER)


def _want(c):
    return (np.frombuffer(c.bases.encode(), U8), np.array(c.offsets, U64), np.array(c.path_offsets, U64), np.array(c.path, U32),
            np.array(c.abund, U64), np.array(c.flags, U8))


def _sizes(c):
    return c.summary[0], c.summary[1], c.summary[7]


def _equal(got, want, ctx):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (ctx, name, g.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g != w)[:5]
        assert not len(bad), (ctx, name, bad, g[bad], w[bad])


def _size(kmc, kc, lo, hi, mr, ms):
    """the sizing call: every array NULL"""
    n = [C.c_uint64(12345) for _ in range(3)]
    w = (C.c_uint64 * kmc.CONTIG_WORDS)()
    kc._chk(kmc.lib().kmc_unitig_contigs(kc._h, lo, hi, mr, ms, None, 0, None, None, None, None, 0, None, 0, *[C.byref(x) for x in n], w))
    return tuple(x.value for x in n), list(w)


def _raw(kmc, kc, lo, hi, mr, ms, sizes, spare=3):
    """kmc_unitig_contigs through ctypes into arrays with `spare` entries more than needed, filled with a pattern"""
    nc, nn, nb = sizes
    bases, flags = np.full(nb + spare, 0xEE, U8), np.full(nc + spare, 0xEE, U8)
    offs, poffs, abund = np.full(nc + 1 + spare, 0xEEEE, U64), np.full(nc + 1 + spare, 0xEEEE, U64), np.full(nc + spare, 0xEEEE, U64)
    path = np.full(nn + spare, 0xEEEE, U32)
    n = [C.c_uint64(12345) for _ in range(3)]
    w = (C.c_uint64 * kmc.CONTIG_WORDS)()
    kc._chk(kmc.lib().kmc_unitig_contigs(kc._h, lo, hi, mr, ms, bases.ctypes.data, nb + spare, offs.ctypes.data, poffs.ctypes.data, abund.ctypes.data,
                                         flags.ctypes.data, nc + spare, path.ctypes.data, nn + spare, *[C.byref(x) for x in n], w))
    assert tuple(x.value for x in n) == sizes
    assert (bases[nb:] == 0xEE).all() and (flags[nc:] == 0xEE).all() and (offs[nc + 1:] == 0xEEEE).all() and (poffs[nc + 1:] == 0xEEEE).all()
    assert (abund[nc:] == 0xEEEE).all() and (path[nn:] == 0xEEEE).all()
    return (bases[:nb], offs[:nc + 1], poffs[:nc + 1], path[:nn], abund[:nc], flags[:nc]), list(w)


def _device(kc, lo, hi, mr, ms):
    """the device form, read back"""
    db, do, dp, dn, da, df, nc, nn, nb, s = kc.contigs_device(lo, hi, mr, ms)
    assert db % 16 == 0 and do % 8 == 0 and dp % 8 == 0 and da % 8 == 0 and dn % 4 == 0
    return (_dev_bytes(db, nb), _dev_u64(do, nc + 1), _dev_u64(dp, nc + 1), _dev_bytes(dn, 4 * nn).view(U32), _dev_u64(da, nc), _dev_bytes(df, nc)), \
        (nc, nn, nb), s.words()


def _forms(kmc, kc, lo, hi, mr, ms, c, ctx):
    """every form of the call against the model's Contigs c"""
    want, words, sizes = _want(c), c.summary, _sizes(c)
    got_sizes, w = _size(kmc, kc, lo, hi, mr, ms)
    assert (got_sizes, w) == (sizes, words), (ctx, got_sizes, sizes, w, words)
    got, w = _raw(kmc, kc, lo, hi, mr, ms, sizes)
    assert w == words, (ctx, w, words)
    _equal(got, want, ctx + ("host",))
    got, dsz, w = _device(kc, lo, hi, mr, ms)
    assert (dsz, w) == (sizes, words), (ctx, dsz, sizes, w, words)
    _equal(got, want, ctx + ("device",))
    r = kc.contigs(lo, hi, mr, ms)
    _equal((r.bases, r.offsets, r.path_offsets, r.path, r.abund, r.flags), want, ctx + ("contigs",))
    assert r.summary.words() == words and len(r) == sizes[0] and r.strings() == c.seqs and r.to_text() == c.text() and r.walks() == c.walks(), ctx


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("name,k", ci.cases())
def test_every_form_against_the_model(kmc, oracle, name, k, canonical):
    case = ci.make(name, k)
    kc, table = _counter(kmc, oracle, case.sample, k, canonical)
    bases, offs = mi.pack(case.reads)
    resolved = 0
    with kc:
        for lo, hi in RANGES:
            t = tm.transits(table, canonical, [case.reads], lo, hi, k=k)
            u = um.unitigs(table, canonical, lo, hi)
            kc.transits(bases, offs, lo, hi)
            for mr in MIN_READS:
                for ms in MIN_SUPPORT:
                    c = cm.Contigs(t, u, mr, ms)
                    _forms(kmc, kc, lo, hi, mr, ms, c, (name, k, canonical, lo, hi, mr, ms))
                    resolved += c.summary[2]
            if name == "tangle":
                _forms(kmc, kc, lo, hi, 1, 2, cm.Contigs(t, u, 1, 2), (name, k, canonical, lo, hi, 1, 2))
            _forms(kmc, kc, lo, hi, 0, 0, cm.Contigs(t, u, 0, 0), (name, k, canonical, lo, hi, 0, 0))       # min_reads 0 is 1
    if name in ci.SPELL_GENOMES and k >= 31:
        assert resolved > 0


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("name,k", [("ladder", 31), ("ladder", 32), ("ladder", 63), ("chain_circular", 31), ("plasmids", 33), ("tangle", 5), ("tangle", 6),
                                    ("hairpin", 31)])
def test_nothing_resolved_is_the_unitigs_byte_for_byte(kmc, oracle, name, k, canonical):
    """min_reads no slot reaches, min_support 0: the device bases, offsets, abund and flags are those of kmc_unitigs_device"""
    case = ci.make(name, k)
    kc, table = _counter(kmc, oracle, case.sample, k, canonical)
    with kc:
        for lo, hi in RANGES:
            kc.transits(*mi.pack(case.reads), lo, hi)
            db, do, da, df, nu, nb, us = kc.unitigs_device(lo, hi)                # (computes again: the links and transits go)
            want = (_dev_bytes(db, nb), _dev_u64(do, nu + 1), _dev_u64(da, nu), _dev_bytes(df, nu))
            kc.transits(*mi.pack(case.reads), lo, hi)
            got, sizes, w = _device(kc, lo, hi, NEVER, 0)
            assert sizes == (nu, nu, nb) and w[2:4] == [0, 0] and w[4] == us.circular
            for name_, g, x in zip(("bases", "offsets", "abund", "flags"), (got[0], got[1], got[4], got[5]), want):
                assert np.array_equal(g, x), (name, k, canonical, lo, hi, name_)
            assert np.array_equal(got[3], 2 * np.arange(nu, dtype=U32)) and np.array_equal(got[2], np.arange(nu + 1, dtype=U64))


def test_accumulation(kmc, oracle):
    k = 31
    case = ci.make("two_repeats", k)
    kc, table = _counter(kmc, oracle, case.sample, k, True)
    u = um.unitigs(table, True)
    half = len(case.reads) // 2
    parts = [case.reads[:half], case.reads[half:]]
    mr = 8
    first = cm.Contigs(tm.transits(table, True, parts[:1], min_reads=mr), u, mr, 1)
    both = cm.Contigs(tm.transits(table, True, parts, min_reads=mr), u, mr, 1)
    assert first.summary != both.summary
    with kc:
        kc.transits(*mi.pack(parts[0]), min_reads=mr)
        _forms(kmc, kc, 1, 0, mr, 1, first, ("first",))
        # one more accumulated batch: the held contigs are dropped, the next call computes again
        kc.transits(*mi.pack(parts[1]), min_reads=mr, accumulate=True)
        _forms(kmc, kc, 1, 0, mr, 1, both, ("both",))
        # two batches, then the first contigs call
        kc.transits(*mi.pack(parts[0]), min_reads=mr)
        kc.transits(*mi.pack(parts[1]), min_reads=mr, accumulate=True)
        _forms(kmc, kc, 1, 0, mr, 1, both, ("both again",))


def test_a_sizing_call_and_the_copy_call_compute_once(kmc, oracle, capfd):
    """seen through the KMC_UNITIG_TRACE line, which a call that computes prints"""
    k = 31
    case = ci.make("repeat", k)
    kc, table = _counter(kmc, oracle, case.sample, k, True)
    c = cm.contigs(table, True, [case.reads])
    with kc:
        kc.transits(*mi.pack(case.reads))
        os.environ["KMC_UNITIG_TRACE"] = "1"
        try:
            capfd.readouterr()
            sizes, _ = _size(kmc, kc, 1, 0, 1, 0)
            _raw(kmc, kc, 1, 0, 1, 0, sizes)
            lines = [x for x in capfd.readouterr().err.splitlines() if x.startswith("kmc_unitig_contigs:")]
            assert len(lines) == 1
            f = lines[0].split()
            assert f[1:10:2] == ["unitigs", "nodes", "contigs", "bases", "rounds"] and f[11::2] == ["choice_ms", "rank_ms", "layout_ms", "emit_ms"]
            assert [int(x) for x in f[2:9:2]] == [5] + [c.summary[i] for i in (1, 0, 7)] and 1 <= int(f[10]) <= 5
            _size(kmc, kc, 1, 0, 2, 0)                                             # other parameters: computes
            _device(kc, 1, 0, 2, 0)                                                # the device form: always
            assert len([x for x in capfd.readouterr().err.splitlines() if x.startswith("kmc_unitig_contigs:")]) == 2
        finally:
            os.environ.pop("KMC_UNITIG_TRACE", None)


@pytest.mark.parametrize("name", ["chain", "chain_circular"])
def test_ranking_rounds_of_a_long_chain(kmc, oracle, capfd, name):
    """contigs of 261 / 260 nodes need 9 doubling rounds at least, and no ranking launches more than ceil(log2(2 n_nodes)) + 1;
    a cycle is ranked twice, before and behind the cut"""
    k = 31
    case = ci.make(name, k)
    kc, table = _counter(kmc, oracle, case.sample, k, True)
    c = cm.contigs(table, True, [case.reads])
    n2 = 2 * c.summary[1]
    bound = 1 + (n2 - 1).bit_length()                       # ceil(log2(n2)) + 1
    assert c.summary[6] in (260, 261) and bound == 12
    with kc:
        kc.transits(*mi.pack(case.reads))
        os.environ["KMC_UNITIG_TRACE"] = "1"
        try:
            capfd.readouterr()
            got, sizes, w = _device(kc, 1, 0, 1, 0)
            lines = [x for x in capfd.readouterr().err.splitlines() if x.startswith("kmc_unitig_contigs:")]
        finally:
            os.environ.pop("KMC_UNITIG_TRACE", None)
    _equal(got, _want(c), (name,))
    assert len(lines) == 1
    rounds = int(lines[0].split()[10])
    rankings = 2 if name == "chain_circular" else 1
    # (the ranking before the cut ends as soon as a round repeats its predecessor's count: one round at least)
    assert 9 + (rankings - 1) <= rounds <= bound * rankings, lines[0]


def test_state_and_argument_errors(kmc, oracle):
    L = kmc.lib()
    k = 31
    case = ci.make("repeat", k)
    bases, offs = mi.pack(case.reads)
    n = [C.c_uint64(9) for _ in range(3)]
    w = (C.c_uint64 * 8)(*([7] * 8))
    tail = lambda: [C.byref(x) for x in n] + [w]
    sizing = lambda h, lo=1, hi=0: L.kmc_unitig_contigs(h, lo, hi, 1, 0, None, 0, None, None, None, None, 0, None, 0, *tail())
    dev = lambda h, lo=1, hi=0: L.kmc_unitig_contigs_device(h, lo, hi, 1, 0, None, None, None, None, None, None, None, None, None, None)
    err = lambda h: L.kmc_last_error(h).decode()
    with kmc.KmerCounter(k=k) as kc:
        # no view
        assert sizing(kc._h) == kmc.ERR_STATE and dev(kc._h) == kmc.ERR_STATE
        # an empty view: nothing held, then zeros
        kc.finalize()
        assert sizing(kc._h) == kmc.ERR_STATE and "unitigs" in err(kc._h)
        kc.transits(bases, offs)
        r = kc.contigs()
        assert r.summary.words() == [0] * 8 and list(r.offsets) == [0] and list(r.path_offsets) == [0] and not len(r.bases) and r.to_text() == ""
        o, p = np.full(4, 0xEEEE, U64), np.full(4, 0xEEEE, U64)
        assert L.kmc_unitig_contigs(kc._h, 1, 0, 1, 0, None, 0, o.ctypes.data, p.ctypes.data, None, None, 0, None, 0, *tail()) == 0
        assert list(o) == list(p) == [0, 0xEEEE, 0xEEEE, 0xEEEE] and [x.value for x in n] == [0, 0, 0] and list(w) == [0] * 8
        assert dev(kc._h) == 0
    kc, table = _counter(kmc, oracle, case.sample, k, True)
    c = cm.contigs(table, True, [case.reads])
    sizes = nc, nn, nb = _sizes(c)
    with kc:
        # what is held, step by step: the message names the missing one
        kc.finalize()
        assert sizing(kc._h) == kmc.ERR_STATE and "unitigs" in err(kc._h)
        kc.unitigs()
        assert dev(kc._h) == kmc.ERR_STATE and "links" in err(kc._h)
        kc.unitig_links()
        assert sizing(kc._h) == kmc.ERR_STATE and "transits" in err(kc._h) and [x.value for x in n] == [0, 0, 0]
        kc.transits(bases, offs)
        assert sizing(kc._h) == 0 and tuple(x.value for x in n) == sizes and list(w) == c.summary
        # transits of another range
        assert sizing(kc._h, 2, 0) == kmc.ERR_STATE and dev(kc._h, 2, 0) == kmc.ERR_STATE
        # a kmc_graph call of another range in between rewrites work arrays, not results
        kc.graph(2, 0, adj=False)
        _forms(kmc, kc, 1, 0, 1, 0, c, ("behind kmc_graph",))
        # arguments
        assert sizing(None) == kmc.ERR_ARG and dev(None) == kmc.ERR_ARG
        assert sizing(kc._h, 3, 2) == kmc.ERR_ARG and dev(kc._h, 3, 2) == kmc.ERR_ARG
        # every cap one too small: KMC_ERR_ARG, the sizes are set and nothing is written
        arr = {"bases": np.full(nb, 0xEE, U8), "offs": np.full(nc + 1, 0xEEEE, U64), "poffs": np.full(nc + 1, 0xEEEE, U64),
               "abund": np.full(nc, 0xEEEE, U64), "flags": np.full(nc, 0xEE, U8), "path": np.full(nn, 0xEEEE, U32)}
        fill = {"bases": 0xEE, "flags": 0xEE}
        for cb, cc, cn, given in ((nb - 1, nc, nn, "all"), (nb, nc - 1, nn, "all"), (nb, nc, nn - 1, "all"), (nb, nc - 1, nn, "offs"),
                                  (nb, nc - 1, nn, "poffs"), (nb, nc - 1, nn, "abund"), (nb, nc - 1, nn, "flags")):
            p = lambda name: arr[name].ctypes.data if given in ("all", name) else None
            rc = L.kmc_unitig_contigs(kc._h, 1, 0, 1, 0, p("bases"), cb, p("offs"), p("poffs"), p("abund"), p("flags"), cc, p("path"), cn, *tail())
            assert rc == kmc.ERR_ARG and tuple(x.value for x in n) == sizes, (cb, cc, cn, given, rc)
            assert all((a == fill.get(name, 0xEEEE)).all() for name, a in arr.items())
        # ... and an array that is NULL has no cap
        assert L.kmc_unitig_contigs(kc._h, 1, 0, 1, 0, None, 0, None, None, None, None, 0, arr["path"].ctypes.data, nn, *tail()) == 0
        assert list(arr["path"]) == c.path and list(w) == c.summary
        # after a finalize that makes a new view, after a reset
        kc.add_batch(*mi.pack(case.sample))
        kc.finalize()
        assert sizing(kc._h) == kmc.ERR_STATE and dev(kc._h) == kmc.ERR_STATE and "unitigs" in err(kc._h)
        kc.transits(bases, offs)
        assert sizing(kc._h) == 0
        kc.reset()
        assert sizing(kc._h) == kmc.ERR_STATE and dev(kc._h) == kmc.ERR_STATE
    with kmc.KmerCounter(mode=kmc.MODE_LR) as lr:
        assert sizing(lr._h) == kmc.ERR_ARG and dev(lr._h) == kmc.ERR_ARG


def test_nothing_else_is_rewritten(kmc, oracle):
    """device pointers handed out earlier by the unitigs, links, map and transits calls read back the same bytes after a contigs call"""
    import torch
    k = 31
    case = ci.make("ladder", k)
    kc, table = _counter(kmc, oracle, case.sample, k, True)
    bases, offs = mi.pack(case.reads)
    dev = torch.device("cuda", 0)
    db = torch.zeros(len(bases) + 64, dtype=torch.uint8, device=dev)
    db[:len(bases)] = torch.from_numpy(bases.copy())
    do = torch.from_numpy(offs.view(np.int64).copy()).to(dev)
    torch.cuda.synchronize(dev)
    with kc:
        ub, uo, ua, uf, nu, nb, _ = kc.unitigs_device()
        lo_, lt, _, nl, _ = kc.unitig_links_device()
        ts, to, tc, tv, _, _, nsl, _ = kc.transits_device(db.data_ptr(), do.data_ptr(), len(offs) - 1, len(bases))
        mp, mr, mo, mg, mu, ns, _, _ = kc.map_reads_device(db.data_ptr(), do.data_ptr(), len(offs) - 1, len(bases))   # (leaves the transits alone)
        held = lambda: [_dev_bytes(ub, nb), _dev_u64(uo, nu + 1), _dev_u64(ua, nu), _dev_bytes(uf, nu), _dev_u64(lo_, 2 * nu + 1), _dev_bytes(lt, 4 * nl),
                        _dev_u64(ts, nl), _dev_u64(to, nu + 1), _dev_u64(tc, nsl), _dev_bytes(tv, nu),
                        _dev_u64(mp, len(bases)), _dev_bytes(mr, 16 * (len(offs) - 1)), _dev_u64(mo, len(offs)), _dev_bytes(mg, 16 * ns), _dev_u64(mu, nu)]
        before = held()
        view = kc.export_device()
        for mr_, ms in ((1, 0), (1, 1), (NEVER, 0)):
            kc.contigs(1, 0, mr_, ms)
            kc.contigs_device(1, 0, mr_, ms)
        assert kc.export_device() == view
        for i, (a, b) in enumerate(zip(before, held())):
            assert np.array_equal(a, b), i
        # ... and the work arrays are still the unitigs': a map call behind it finds them and computes nothing again
        r = kc.map_reads(bases, offs)
        assert np.array_equal(before[0], _dev_bytes(ub, nb)) and r.summary.crossings > 0


@pytest.mark.parametrize("canonical", [True, False])
def test_round_trip_into_a_second_counter(kmc, oracle, canonical):
    """d_bases / d_offsets into kmc_add_batch_device of a second ctx: its key set is the first view's.  A contig may be spelled
    on the other strand (it starts at its end node with the smaller id), so the second ctx counts canonical k-mers; behind a
    canonical first ctx its table is the first view, behind a forward one the canonical table of the same sample."""
    k = 31
    case = ci.make("two_repeats", k)
    kc, table = _counter(kmc, oracle, case.sample, k, canonical)
    with kc, kmc.KmerCounter(k=k, canonical=True) as other:
        kc.transits(*mi.pack(case.reads))
        db, do, _, _, _, _, nc, nn, nb, s = kc.contigs_device()
        assert s.unitigs_duplicated == 2 and nc == 2
        other.add_batch_device(db, do, nc, nb)
        got, first = other.export(), kc.export()
        want = first if canonical else oracle.count_kmers(*mi.pack(case.sample), k, True)
        assert np.array_equal(got.key_hi, want.key_hi) and np.array_equal(got.key_lo, want.key_lo)
        # the contigs are the two genomes, so counting them again gives the very table: the repeats' keys once per copy
        assert int(got.count.sum()) == nb - nc * (k - 1) and got.equals(want)


@pytest.mark.parametrize("name", ["repeat", "plasmids"])
def test_cli_contigs(kmc, tmp_path, name):
    k = 31
    case = ci.make(name, k)
    sample, reads = str(tmp_path / "sample.fa"), str(tmp_path / "reads.fa")
    for path, seqs in ((sample, case.sample), (reads, case.reads)):
        with open(path, "w") as f:
            f.write("".join(">%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    for canonical in (True, False):
        table = gm.count_table(case.sample, k, canonical)
        fw = [] if canonical else ["--forward"]
        run = lambda *a: subprocess.run([EXE, sample, "-k", str(k), "--contigs", reads] + list(a) + fw, capture_output=True, text=True)
        r = run()
        assert r.returncode == 0 and r.stdout == cm.contigs(table, canonical, [case.reads]).text() and r.stdout.count("\n>") == 1, r.stderr
        r = run("--min-reads", str(ti.PAIR_DEPTH + 1), "--min-support", "3")
        assert r.returncode == 0 and r.stdout == cm.contigs(table, canonical, [case.reads], min_reads=ti.PAIR_DEPTH + 1, min_support=3).text(), r.stderr
