"""GPU checks of kmc_unitig_transits / kmc_unitig_transits_device / KmerCounter.transits (kmc_transits.hip.h).  Expected values
come from tests/transit_model.py -- the definitions of include/kmc.h over Python lists, on top of map_model's segments and
links_model's records -- applied to the CPU oracle's table of the same input.  All comparisons are exact, array by array,
through every form of the call."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import bubble_model as bm
import graph_model as gm
import map_inputs as mi
import transit_inputs as ti
import transit_model as tm
from conftest import ROOT, SAMPLE
from test_map_gpu import _counter, _sample_reads
from test_unitig_gpu import _dev_bytes, _dev_u64

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "bin", "k-mer-count")
U64, U8 = np.uint64, np.uint8
KS = (5, 6, 31, 32, 33, 63)
NAMES = ("link_support", "transit_offsets", "transit_count", "verdict")


def _want(t):
    return (np.array(t.link_support, U64), np.array(t.transit_offsets, U64), np.array(t.transit_count, U64), np.array(t.verdict, U8))


def _sizes(t):
    return len(t.verdict), len(t.link_support), len(t.transit_count)


def _equal(got, want, ctx):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (ctx, name, g.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g != w)[:5]
        assert not len(bad), (ctx, name, bad, g[bad], w[bad])


def _size(kmc, kc, lo, hi, bases, offs, min_reads=1, flags=0):
    """the sizing call: every array NULL"""
    n = [C.c_uint64(12345) for _ in range(3)]
    w = (C.c_uint64 * kmc.TRANSIT_WORDS)()
    kc._chk(kmc.lib().kmc_unitig_transits(kc._h, lo, hi, min_reads, flags, bases.ctypes.data, offs.ctypes.data, len(offs) - 1, None, 0, None, 0,
                                          None, 0, None, *[C.byref(x) for x in n], w))
    return tuple(x.value for x in n), list(w)


def _raw(kmc, kc, lo, hi, bases, offs, sizes, min_reads=1, flags=0, spare=3):
    """kmc_unitig_transits through ctypes into arrays with `spare` entries more than needed, filled with a pattern"""
    nu, nl, nsl = sizes
    sup, to = np.full(nl + spare, 0xEEEE, U64), np.full(nu + 1 + spare, 0xEEEE, U64)
    cnt, vd = np.full(nsl + spare, 0xEEEE, U64), np.full(nu + spare, 0xEE, U8)
    n = [C.c_uint64(12345) for _ in range(3)]
    w = (C.c_uint64 * kmc.TRANSIT_WORDS)()
    kc._chk(kmc.lib().kmc_unitig_transits(kc._h, lo, hi, min_reads, flags, bases.ctypes.data, offs.ctypes.data, len(offs) - 1, sup.ctypes.data,
                                          nl + spare, to.ctypes.data, nu + spare, cnt.ctypes.data, nsl + spare, vd.ctypes.data,
                                          *[C.byref(x) for x in n], w))
    assert tuple(x.value for x in n) == sizes
    assert (sup[nl:] == 0xEEEE).all() and (to[nu + 1:] == 0xEEEE).all() and (cnt[nsl:] == 0xEEEE).all() and (vd[nu:] == 0xEE).all()
    return (sup[:nl], to[:nu + 1], cnt[:nsl], vd[:nu]), list(w)


def _upload(bases, offs):
    import torch
    dev = torch.device("cuda", 0)
    db = torch.zeros(len(bases) + 64, dtype=torch.uint8, device=dev)
    db[:len(bases)] = torch.from_numpy(bases.copy())
    do = torch.from_numpy(offs.view(np.int64).copy()).to(dev)
    torch.cuda.synchronize(dev)
    return db, do


def _device(kc, lo, hi, bases, offs, min_reads=1, accumulate=False):
    """the device form on an uploaded batch, read back"""
    db, do = _upload(bases, offs)
    ds, dt, dc, dv, nu, nl, nsl, s = kc.transits_device(db.data_ptr(), do.data_ptr(), len(offs) - 1, len(bases), lo, hi, min_reads, accumulate)
    assert ds % 8 == 0 and dt % 8 == 0 and dc % 8 == 0
    return (_dev_u64(ds, nl), _dev_u64(dt, nu + 1), _dev_u64(dc, nsl), _dev_bytes(dv, nu)), (nu, nl, nsl), s.words()


def _check(kmc, kc, table, canonical, reads, ranges=((1, 0), (2, 0)), min_reads=1):
    """every form of the call against the model, for every range; returns {range: the model's Transits}"""
    bases, offs = mi.pack(reads)
    seen = {}
    for lo, hi in ranges:
        t = tm.transits(table, canonical, [reads], lo, hi, min_reads, k=kc.k)
        want, words, sizes = _want(t), t.summary, _sizes(t)
        ctx = (kc.k, canonical, lo, hi, min_reads)
        got_sizes, w = _size(kmc, kc, lo, hi, bases, offs, min_reads)
        assert (got_sizes, w) == (sizes, words), (ctx, got_sizes, sizes, w, words)
        got, w = _raw(kmc, kc, lo, hi, bases, offs, sizes, min_reads)
        assert w == words, (ctx, w, words)
        _equal(got, want, ctx + ("host",))
        got, dsz, w = _device(kc, lo, hi, bases, offs, min_reads)
        assert (dsz, w) == (sizes, words), (ctx, dsz, sizes, w, words)
        _equal(got, want, ctx + ("device",))
        r = kc.transits(bases, offs, lo, hi, min_reads)
        _equal((r.link_support, r.transit_offsets, r.transit_count, r.verdict), want, ctx + ("transits",))
        assert r.summary.words() == words and len(r) == sizes[0] and r.to_text() == t.text(), ctx
        assert list(r.links.offsets) == t.lk.offsets and list(r.links.to) == t.lk.to
        assert words[0] == t.maps[0].summary[4] == kc.map_reads(bases, offs, lo, hi).summary.crossings       # identity [0]
        assert words[3] == int(r.transit_count.sum())
        seen[(lo, hi)] = t
    return seen


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", KS)
def test_constructed_repeats(kmc, oracle, k, canonical):
    """repeat / short / chimera: one 2 x 2 repeat at k >= 31, tangles with up to 4 x 4 matrices at k = 5 and 6, and at k = 6
    canonical the missing-record branches"""
    depth = ti.PAIR_DEPTH if canonical else ti.PAIR_DEPTH // 2
    dropped = most = 0
    for name, verdict in (("repeat", tm.RESOLVED), ("short", tm.UNSPANNED), ("chimera", tm.AMBIGUOUS)):
        sample, reads = getattr(ti, name)(k, 500 + k)
        kc, table = _counter(kmc, oracle, sample, k, canonical)
        with kc:
            t = _check(kmc, kc, table, canonical, reads)[(1, 0)]
            if k >= 31:
                assert sorted(t.verdict) == [tm.PLAIN] * 4 + [verdict], (name, t.verdict)
            if name == "repeat":
                for mr in (0, depth + 1):
                    _check(kmc, kc, table, canonical, reads, ((1, 0),), mr)
                if k >= 31:
                    bases, offs = mi.pack(reads)
                    assert kc.transits(bases, offs, min_reads=depth + 1).summary.words()[5:] == [1, 0, 0]       # UNSPANNED
                    assert kc.transits(bases, offs, min_reads=depth).summary.words()[5:] == [1, 1, 0]
        dropped += t.summary[4]
        most = max([most] + [a * b for a, b in zip(t.d_start, t.d_end)])
    assert most == 4 if k >= 31 else most == 16 if k == 5 else most >= 6              # (the k = 5 tangle has 4 x 4 matrices)
    if canonical and k == 6:
        assert dropped > 0


def _map_inputs(k, canonical):
    out = [("genome", mi.genome_reads(k, 100 + k)), ("circular", mi.circular(k, 200 + k))]
    if k == 31:
        out.append(("two_graphs", mi.two_graphs(k, 10, n_reads=20)))
    if canonical and k % 2 == 1:
        out.append(("hairpin", mi.hairpin(k, 400 + k)))
    return out


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", KS)
def test_inputs_of_the_map_tests(kmc, oracle, k, canonical):
    """both strands, gaps, N; a cycle read twice round (END -> START of one unitig as in- and out-record); segments on both
    sides of the position tiles' seams; a hairpin's crossings with a == b"""
    loops = crossings = 0
    for name, (sample, reads) in _map_inputs(k, canonical):
        kc, table = _counter(kmc, oracle, sample, k, canonical)
        with kc:
            t = _check(kmc, kc, table, canonical, reads, ((1, 0), (2, 0)) if name == "genome" else ((1, 0),))[(1, 0)]
        loops += t.loops
        crossings += t.summary[0]
        if name == "circular" and k >= 31:
            u = [i for i, s in enumerate(t.seqs) if len(s) - k + 1 == 50][0]
            assert 2 * u in t.lk.to[t.lk.offsets[2 * u + 1]:t.lk.offsets[2 * u + 2]] and sum(map(sum, t.matrix(u))) >= 1
    assert crossings > 0 and (loops > 0) == (canonical and k % 2 == 1)


@pytest.mark.parametrize("canonical", [True, False])
def test_a_read_boundary_is_no_crossing(kmc, oracle, canonical):
    """the first segment of a read that starts where the last segment of the read before it ends, in one wave, across a
    wave's edge and across a workgroup's"""
    k = 31
    sample, reads = ti.read_boundary(k, 600)
    kc, table = _counter(kmc, oracle, sample, k, canonical)
    with kc:
        t = _check(kmc, kc, table, canonical, reads, ((1, 0),))[(1, 0)]
    m = t.maps[0]
    at = {m.seg_offsets[r] for r in range(1, len(reads)) if m.seg_offsets[r + 1] > m.seg_offsets[r] and m.segments[m.seg_offsets[r]][0] == 20}
    assert {64, 128, 192, 256} <= at and len(at) >= 200
    assert t.summary[0] == 4 * (ti.PAIR_DEPTH if canonical else ti.PAIR_DEPTH // 2)


def test_hot_link_batch_counts_exactly(kmc, oracle):
    """110 000 reads on eight records and four slots: thousands of lanes add to the same few words.  Every array equals 2 500
    times the single-copy result, with the per-wave combine and without it."""
    k, copies = 31, 2500
    sample, reads = ti.repeat(k, 500 + k)
    kc, table = _counter(kmc, oracle, sample, k, True)
    one = tm.transits(table, True, [reads])
    want = _want(one)
    want = (want[0] * U64(copies), want[1], want[2] * U64(copies), want[3])
    words = [x * copies for x in one.summary[:5]] + one.summary[5:]
    assert len(reads) * copies == 110000 and len(want[0]) == 8 and len(want[2]) == 4 and words[2] == 0
    bases, offs = mi.pack(reads)
    n = len(bases)
    big = np.tile(bases, copies)
    big_offs = np.concatenate([[0], (offs[1:][None, :] + (np.arange(copies, dtype=U64) * U64(n))[:, None]).ravel()]).astype(U64)
    assert len(big_offs) == 110001 and int(big_offs[-1]) == len(big)
    with kc:
        try:
            for plain in (False, True):
                if plain:
                    os.environ["KMC_TRANSITS_PLAIN"] = "1"
                got, sizes, w = _device(kc, 1, 0, big, big_offs)
                assert (sizes, w) == (_sizes(one), words), (plain, sizes, w, words)
                _equal(got, want, ("hot", plain))
        finally:
            os.environ.pop("KMC_TRANSITS_PLAIN", None)
        # ... and the small inputs give the same arrays without the combine
        os.environ["KMC_TRANSITS_PLAIN"] = "1"
        try:
            _equal(_device(kc, 1, 0, bases, offs)[0], _want(one), ("plain",))
        finally:
            os.environ.pop("KMC_TRANSITS_PLAIN", None)


def test_accumulate(kmc, oracle):
    k = 31
    L = kmc.lib()
    sample, reads = ti.chimera(k, 500 + k)
    kc, table = _counter(kmc, oracle, sample, k, True)
    whole = tm.transits(table, True, [reads], min_reads=3)
    parts = [reads[:9], [], reads[9:]]
    packed = [mi.pack(p) for p in parts]
    first = tm.transits(table, True, [parts[0]], min_reads=3)
    last = tm.transits(table, True, [parts[2]], min_reads=3)
    assert tm.transits(table, True, parts, min_reads=3).arrays() == whole.arrays()
    none = lambda flags: L.kmc_unitig_transits_device(kc._h, 1, 0, 3, flags, None, None, 0, 0, None, None, None, None, None, None, None, None)
    with kc:
        # nothing held yet
        assert none(kmc.TRANSIT_ACCUMULATE) == kmc.ERR_STATE and "ACCUMULATE" in L.kmc_last_error(kc._h).decode()
        # three calls, the middle one without a read, through the device form
        got, sizes, w = _device(kc, 1, 0, *packed[0], 3)
        _equal(got, _want(first), "first")
        assert w == first.summary
        got, sizes, w = _device(kc, 1, 0, *packed[1], 3, True)
        _equal(got, _want(first), "middle")
        assert w == first.summary and sizes == _sizes(whole)
        # a map, a profile and a correct call in between do not disturb the totals
        kc.map_reads(*mi.pack(reads))
        kc.profile(*mi.pack(reads))
        kc.correct_reads(*mi.pack(reads))
        got, sizes, w = _device(kc, 1, 0, *packed[2], 3, True)
        _equal(got, _want(whole), "whole")
        assert w == whole.summary
        # the verdict follows this call's min_reads: the totals under min_reads 1
        r = kc.transits(*packed[1], min_reads=1, accumulate=True)
        again = tm.transits(table, True, [reads], min_reads=1)
        _equal((r.link_support, r.transit_offsets, r.transit_count, r.verdict), _want(again), "min_reads 1")
        assert r.summary.words() == again.summary
        # through the host form
        got, w = _raw(kmc, kc, 1, 0, *packed[0], _sizes(whole), 3)
        got, w = _raw(kmc, kc, 1, 0, *packed[2], _sizes(whole), 3, kmc.TRANSIT_ACCUMULATE)
        _equal(got, _want(whole), "host")
        assert w == whole.summary
        # without the flag a call replaces what is held
        got, sizes, w = _device(kc, 1, 0, *packed[2], 3)
        _equal(got, _want(last), "replaced")
        assert w == last.summary
        # another range has nothing held; a kmc_graph call of another range drops what is held (the next call computes the
        # unitigs again); so does a finalize
        assert L.kmc_unitig_transits_device(kc._h, 2, 0, 3, 1, None, None, 0, 0, None, None, None, None, None, None, None, None) == kmc.ERR_STATE
        assert none(kmc.TRANSIT_ACCUMULATE) == 0
        kc.graph(2, 0, adj=False)
        assert none(kmc.TRANSIT_ACCUMULATE) == kmc.ERR_STATE
        assert none(0) == 0 and none(kmc.TRANSIT_ACCUMULATE) == 0
        kc.add_batch(*mi.pack(sample))
        kc.finalize()
        assert none(kmc.TRANSIT_ACCUMULATE) == kmc.ERR_STATE
        got, sizes, w = _device(kc, 1, 0, *mi.pack(reads), 3)
        _equal(got, _want(whole), "after finalize")


def test_a_finalize_with_nothing_added_makes_no_new_view(kmc, oracle):
    """include/kmc.h, kmc_finalize: a call that finds nothing added since the last finalize of a small table reports the view
    in place and drops nothing: the same device pointers, and the held transits are still there to add to (a finalize
    behind an added batch drops them: test_accumulate)"""
    k = 31
    sample, reads = ti.repeat(k, 500 + k)
    kc, table = _counter(kmc, oracle, sample, k, True)
    bases, offs = mi.pack(reads)
    twice = tm.transits(table, True, [reads, reads])
    with kc:
        _device(kc, 1, 0, bases, offs)
        view = kc.export_device()
        assert kc.finalize() == (len(table), sum(table.values())) and kc.export_device() == view
        got, sizes, w = _device(kc, 1, 0, bases, offs, accumulate=True)
        _equal(got, _want(twice), "behind a finalize with nothing added")
        assert w == twice.summary and sizes == _sizes(twice)


_CHILD = r"""
import importlib, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
kmc = importlib.import_module("k-mer-count_amd")
bases, offs = kmc.parse_fasta(sys.argv[2])
arrays = lambda t: (t.link_support, t.transit_offsets, t.transit_count, t.verdict, t.links.offsets, t.links.to)
same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(arrays(a), arrays(b))) and a.summary == b.summary
with kmc.KmerCounter(k=31) as kc:
    kc.add_batch(bases, offs)
    kc.finalize()
    print("step links(1,0)", file=sys.stderr, flush=True)
    u = kc.unitigs(1, 0)
    l1 = kc.unitig_links(1, 0)
    print("step transits(1,0)", file=sys.stderr, flush=True)
    a = kc.transits(bases, offs, 1, 0)
    assert np.array_equal(a.links.offsets, l1.offsets) and np.array_equal(a.links.to, l1.to)
    u2 = kc.unitigs(1, 0)
    assert np.array_equal(u.bases, u2.bases) and np.array_equal(u.offsets, u2.offsets) and np.array_equal(u.abund, u2.abund)
    assert a.summary.crossings == kc.map_reads(bases, offs, 1, 0).summary.crossings > 0
    print("step graph(2,0) transits(1,0)", file=sys.stderr, flush=True)
    kc.graph(2, 0, adj=False)
    b = kc.transits(bases, offs, 1, 0)
    assert same(a, b)
    print("step clean bubbles", file=sys.stderr, flush=True)
    v = kc.clean_unitigs(1, 0)
    bb = kc.bubbles(1, 0)
    print("step transits(1,0) behind them", file=sys.stderr, flush=True)
    c = kc.transits(bases, offs, 1, 0)
    assert same(a, c)
    v2 = kc.clean_unitigs(1, 0)
    bb2 = kc.bubbles(1, 0)
    assert np.array_equal(v.verdict, v2.verdict) and np.array_equal(bb.records, bb2.records)
    print("step end", file=sys.stderr, flush=True)
"""


def test_orderings_through_the_trace_lines(kmc):
    """What computes, seen through the KMC_UNITIG_TRACE lines of a child process (nothing is timed)"""
    env = dict(os.environ, KMC_UNITIG_TRACE="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, SAMPLE], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    steps, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("step "):
            cur = line[5:]
            steps[cur] = []
        elif line.startswith("kmc_"):
            name = line.split(":")[0]
            steps[cur].append(name + (" reused" if name == "kmc_unitig_transits" and "links_reused 1" in line else ""))
    assert steps["links(1,0)"] == ["kmc_unitigs", "kmc_unitig_links"]
    assert steps["transits(1,0)"] == ["kmc_unitig_map", "kmc_unitig_transits reused", "kmc_unitig_map"]       # (the last: the map call it is held against)
    assert steps["graph(2,0) transits(1,0)"] == ["kmc_unitigs", "kmc_unitig_links", "kmc_unitig_map", "kmc_unitig_transits"]
    assert steps["transits(1,0) behind them"] == ["kmc_unitig_map", "kmc_unitig_transits reused"]               # clean and bubbles: copied, not computed
    line = [x for x in r.stderr.splitlines() if x.startswith("kmc_unitig_transits:")][0].split()
    assert line[1:14:2] == ["unitigs", "records", "reads", "segments", "crossings", "transits", "links_reused"]
    assert line[15::2] == ["map_ms", "transit_ms", "verdict_ms"]


def test_empty_inputs_and_errors(kmc, oracle):
    L = kmc.lib()
    k = 31
    sample, reads = ti.chimera(k, 5)
    bases, offs = mi.pack(reads)
    n = [C.c_uint64(9) for _ in range(3)]
    w = (C.c_uint64 * 8)(*([7] * 8))
    tail = lambda: [C.byref(x) for x in n] + [w]
    sizing = lambda h, lo, hi, flags, b, o, nr: L.kmc_unitig_transits(h, lo, hi, 1, flags, b.ctypes.data, o.ctypes.data, nr, None, 0, None, 0, None, 0, None, *tail())
    dev_none = lambda h: L.kmc_unitig_transits_device(h, 1, 0, 1, 0, None, None, 0, 0, None, None, None, None, None, None, None, None)
    with kmc.KmerCounter(k=k) as kc:
        # no view
        assert sizing(kc._h, 1, 0, 0, bases, offs, len(reads)) == kmc.ERR_STATE and dev_none(kc._h) == kmc.ERR_STATE
        # an empty view: transit_offsets[0] == 0 and zeros
        kc.finalize()
        r = kc.transits(bases, offs)
        assert r.summary.words() == [0] * 8 and list(r.transit_offsets) == [0] and not len(r.link_support) and not len(r.verdict) and r.to_text() == ""
        to = np.full(4, 0xEEEE, U64)
        assert L.kmc_unitig_transits(kc._h, 1, 0, 1, 0, bases.ctypes.data, offs.ctypes.data, len(reads), None, 0, to.ctypes.data, 0, None, 0, None, *tail()) == 0
        assert list(to) == [0, 0xEEEE, 0xEEEE, 0xEEEE] and [x.value for x in n] == [0, 0, 0] and list(w) == [0] * 8
    kc, table = _counter(kmc, oracle, sample, k, True)
    t = tm.transits(table, True, [reads])
    sizes = nu, nl, nsl = _sizes(t)
    assert nu > 1 and nl > 1 and nsl > 1
    with kc:
        # no reads: the sizes, zeroed arrays, PLAIN or UNSPANNED
        z = np.zeros(1, U64)
        r = kc.transits(np.zeros(0, U8), z)
        zero = tm.transits(table, True, [[]])
        _equal((r.link_support, r.transit_offsets, r.transit_count, r.verdict), _want(zero), "no reads")
        assert r.summary.words() == zero.summary == [0, 0, nl, 0, 0, 1, 0, 0]
        assert L.kmc_unitig_transits(kc._h, 1, 0, 1, 0, None, None, 0, None, 0, None, 0, None, 0, None, *tail()) == 0
        assert [x.value for x in n] == list(sizes) and list(w) == zero.summary
        # arguments
        assert sizing(None, 1, 0, 0, bases, offs, len(reads)) == kmc.ERR_ARG
        assert sizing(kc._h, 3, 2, 0, bases, offs, len(reads)) == kmc.ERR_ARG
        assert sizing(kc._h, 1, 0, 2, bases, offs, len(reads)) == kmc.ERR_ARG and "flag" in L.kmc_last_error(kc._h).decode()
        assert sizing(kc._h, 1, 0, 0x80000001, bases, offs, len(reads)) == kmc.ERR_ARG
        bad = offs.copy()
        bad[3] = bad[2] - 1
        assert sizing(kc._h, 1, 0, 0, bases, bad, len(reads)) == kmc.ERR_ARG
        # every cap one too small: KMC_ERR_ARG, the sizes are set and nothing is written
        sup, to, cnt, vd = np.full(nl, 0xEEEE, U64), np.full(nu + 1, 0xEEEE, U64), np.full(nsl, 0xEEEE, U64), np.full(nu, 0xEE, U8)
        for cl, cu, cs, arrays in ((nl - 1, nu, nsl, "all"), (nl, nu - 1, nsl, "all"), (nl, nu, nsl - 1, "all"), (nl, nu - 1, nsl, "verdict")):
            p = lambda a, name: a.ctypes.data if arrays == "all" or arrays == name else None
            rc = L.kmc_unitig_transits(kc._h, 1, 0, 1, 0, bases.ctypes.data, offs.ctypes.data, len(reads), p(sup, "sup"), cl, p(to, "to"), cu,
                                       p(cnt, "cnt"), cs, p(vd, "verdict"), *tail())
            assert rc == kmc.ERR_ARG and [x.value for x in n] == list(sizes), (cl, cu, cs, rc)
            assert (sup == 0xEEEE).all() and (to == 0xEEEE).all() and (cnt == 0xEEEE).all() and (vd == 0xEE).all()
        # ... and an array that is NULL has no cap
        assert L.kmc_unitig_transits(kc._h, 1, 0, 1, 0, bases.ctypes.data, offs.ctypes.data, len(reads), sup.ctypes.data, nl, None, 0, None, 0, None,
                                     *tail()) == 0
        assert np.array_equal(sup, np.array(t.link_support, U64)) and list(w) == t.summary
    with kmc.KmerCounter(mode=kmc.MODE_LR) as lr:
        assert sizing(lr._h, 1, 0, 0, bases, offs, len(reads)) == kmc.ERR_ARG and dev_none(lr._h) == kmc.ERR_ARG


@pytest.mark.parametrize("forward", [False, True])
def test_cli_transits(kmc, forward):
    k, canonical = 31, not forward
    reads = _sample_reads(kmc)
    table = gm.count_table(reads, k, canonical)
    fw = ["--forward"] if forward else []
    run = lambda *a: subprocess.run([EXE, SAMPLE, "-k", str(k), "--transits", SAMPLE] + list(a) + fw, capture_output=True, text=True)
    want = tm.transits(table, canonical, [reads])
    r = run()
    assert r.returncode == 0 and r.stdout == want.text() and r.stdout.count("L\t") > 0, r.stderr
    r = run("--min-count", "2", "--min-reads", "2")
    assert r.returncode == 0 and r.stdout == tm.transits(table, canonical, [reads], 2, 0, 2).text(), r.stderr
    if not forward:
        final = bm.rounds(table, canonical, max_bubble=31, n_rounds=1)[0]
        r = run("--clean", "1", "--bubble-keys", "31")
        assert r.returncode == 0 and r.stdout == tm.transits(final, canonical, [reads], k=k).text(), r.stderr
