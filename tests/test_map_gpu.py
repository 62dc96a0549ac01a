"""GPU checks of kmc_unitig_map / kmc_unitig_map_device / KmerCounter.map_reads (kmc_map.hip.h).  Expected values come from
tests/map_model.py -- the definitions of include/kmc.h on Python strings, on top of unitig_model's spellings -- applied to
the CPU oracle's table of the same input.  All comparisons are exact, entry by entry, through every form of the call."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import bubble_model as bm
import graph_model as gm
import map_inputs as mi
import map_model as mm
import unitig_model as um
from conftest import ROOT, SAMPLE
from test_unitig_gpu import _dev_bytes, _dev_u64, _table_dict

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "bin", "k-mer-count")
U64, U32 = np.uint64, np.uint32
RANGES = ((1, 0), (2, 0), (1, 1), (2, 3))
NAMES = ("place", "stats", "seg_offsets", "segments", "support")


def _want(m):
    return (np.array(m.place, U64), np.array(m.stats, U32).reshape(-1, 4), np.array(m.seg_offsets, U64),
            np.array(m.segments, U32).reshape(-1, 4), np.array(m.support, U64))


def _equal(got, want, ctx):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.size == w.size, (ctx, name, g.dtype, g.shape, w.shape)
        g = g.reshape(w.shape)
        bad = np.flatnonzero((g != w).reshape(len(w), -1).any(axis=1))[:5] if w.size else []
        assert not len(bad), (ctx, name, bad, g[bad], w[bad])


def _raw(kmc, kc, lo, hi, bases, offs, ns, nu, spare=3):
    """kmc_unitig_map through ctypes into arrays with `spare` entries more than needed, filled with a pattern"""
    L = kmc.lib()
    nr, nb = len(offs) - 1, len(bases)
    place, stats = np.full(nb + spare, 0xEEEE, U64), np.full(4 * nr + spare, 0xEEEEEEEE, U32)
    so, segs, sup = np.full(nr + 1 + spare, 0xEEEE, U64), np.full(4 * (ns + spare), 0xEEEEEEEE, U32), np.full(nu + spare, 0xEEEE, U64)
    n1, n2 = C.c_uint64(12345), C.c_uint64(12345)
    w = (C.c_uint64 * kmc.MAP_WORDS)()
    kc._chk(L.kmc_unitig_map(kc._h, lo, hi, bases.ctypes.data, offs.ctypes.data, nr, place.ctypes.data, stats.ctypes.data, so.ctypes.data,
                             segs.ctypes.data, ns + spare, sup.ctypes.data, nu + spare, C.byref(n1), C.byref(n2), w))
    assert (n1.value, n2.value) == (ns, nu)
    assert (place[nb:] == 0xEEEE).all() and (stats[4 * nr:] == 0xEEEEEEEE).all() and (so[nr + 1:] == 0xEEEE).all()
    assert (segs[4 * ns:] == 0xEEEEEEEE).all() and (sup[nu:] == 0xEEEE).all()
    return (place[:nb], stats[:4 * nr], so[:nr + 1], segs[:4 * ns], sup[:nu]), list(w)


def _device(kc, lo, hi, bases, offs):
    """the device form on an uploaded batch, read back"""
    import torch
    dev = torch.device("cuda", 0)
    nr, nb = len(offs) - 1, len(bases)
    db = torch.zeros(nb + 64, dtype=torch.uint8, device=dev)
    db[:nb] = torch.from_numpy(bases.copy())
    do = torch.from_numpy(offs.view(np.int64).copy()).to(dev)
    torch.cuda.synchronize(dev)
    dp, ds, dso, dg, du, ns, nu, s = kc.map_reads_device(db.data_ptr(), do.data_ptr(), nr, nb, lo, hi)
    assert dp % 8 == 0 and ds % 16 == 0 and dso % 8 == 0 and dg % 16 == 0 and du % 8 == 0
    got = (_dev_u64(dp, nb), _dev_bytes(ds, 16 * nr).view(U32), _dev_u64(dso, nr + 1), _dev_bytes(dg, 16 * ns).view(U32), _dev_u64(du, nu))
    return got, ns, nu, s.words()


def _check(kmc, kc, table, canonical, reads, ranges=RANGES):
    """every form of the call against the model, for every range; returns {range: the model's ReadMap}"""
    L = kmc.lib()
    bases, offs = mi.pack(reads)
    seen = {}
    for lo, hi in ranges:
        m = mm.map_reads(table, canonical, reads, lo, hi, k=kc.k)
        want, words = _want(m), m.summary
        ns, nu = words[3], m.n_unitigs
        ctx = (kc.k, canonical, lo, hi)
        # the sizing call
        n1, n2 = C.c_uint64(1), C.c_uint64(1)
        w = (C.c_uint64 * 8)()
        kc._chk(L.kmc_unitig_map(kc._h, lo, hi, bases.ctypes.data, offs.ctypes.data, len(reads), None, None, None, None, 0, None, 0,
                                 C.byref(n1), C.byref(n2), w))
        assert (n1.value, n2.value, list(w)) == (ns, nu, words), (ctx, n1.value, n2.value, list(w), words)
        got, w = _raw(kmc, kc, lo, hi, bases, offs, ns, nu)
        assert w == words, (ctx, w, words)
        _equal(got, want, ctx + ("host",))
        got, dns, dnu, w = _device(kc, lo, hi, bases, offs)
        assert (dns, dnu, w) == (ns, nu, words), (ctx, dns, dnu, w, words)
        _equal(got, want, ctx + ("device",))
        r = kc.map_reads(bases, offs, lo, hi)
        _equal((r.place, r.stats, r.seg_offsets, r.segments, r.support), want, ctx + ("map_reads",))
        assert r.summary.words() == words and len(r) == len(reads) and r.walks() == m.walks()
        assert "".join("%d\t%d\t%d\t%d\t%s\n" % (i, r.stats[i][0], r.stats[i][1], r.stats[i][2], r.walk_text(i)) for i in range(len(r))) == m.text()
        assert words[2] == int(r.support.sum()) and words[3] == int(r.seg_offsets[-1])
        seen[(lo, hi)] = m
    return seen


def _counter(kmc, oracle, sample, k, canonical):
    bases, offs = mi.pack(sample)
    want = oracle.count_kmers(bases, offs, k, canonical)
    table = _table_dict(want)
    assert table == gm.count_table(sample, k, canonical)
    kc = kmc.KmerCounter(k=k, canonical=canonical)
    kc.add_batch(bases, offs)
    assert kc.export().equals(want)
    return kc, table


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [5, 6, 31, 32, 33, 63])
def test_reads_mapped_back_and_gaps(kmc, oracle, k, canonical):
    """key widths and parities; both strands; N, lower case, short and empty reads; a second sample with substitutions"""
    sample, reads = mi.genome_reads(k, 100 + k)
    kc, table = _counter(kmc, oracle, sample, k, canonical)
    with kc:
        seen = _check(kmc, kc, table, canonical, reads)
    w = seen[(1, 0)].summary
    assert w[1] > w[2] > 0 and w[4] > 0 and w[5] > 0 and w[6] >= 5, w
    if k >= 31:     # (at k = 5 and 6 the sample fills the k-mer space: those check exactness alone)
        assert any(s[2] & 1 for s in seen[(1, 0)].segments) == canonical
        assert seen[(2, 0)].summary[2] < w[2]                    # windows that are valid and not solid


@pytest.mark.parametrize("canonical", [True, False])
def test_one_segment_across_chunks_and_a_waves_span(kmc, oracle, canonical):
    k = 31
    sample, reads = mi.one_long_unitig(k, 7)
    kc, table = _counter(kmc, oracle, sample, k, canonical)
    with kc:
        m = _check(kmc, kc, table, canonical, reads, ((1, 0),))[(1, 0)]
    assert um.unitigs(table, canonical).summary[5] > 2100
    assert m.stats[0] == [2970, 2970, 1, 0] and m.stats[2][2] == 1
    assert m.stats[1] == ([2970, 2970, 1, 0] if canonical else [2970, 0, 0, 0])


@pytest.mark.parametrize("canonical", [True, False])
def test_segments_on_both_sides_of_every_tile_edge(kmc, oracle, canonical):
    k = 31
    sample, reads = mi.two_graphs(k, 10)
    kc, table = _counter(kmc, oracle, sample, k, canonical)
    with kc:
        m = _check(kmc, kc, table, canonical, reads, ((1, 0), (2, 0)))[(1, 0)]
    assert m.summary[3] >= 500 and len(m.place) > 20 * 2048 and m.summary[7] >= 5


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [6, 31, 32])
def test_circular_unitigs(kmc, oracle, k, canonical):
    sample, reads = mi.circular(k, 200 + k)
    kc, table = _counter(kmc, oracle, sample, k, canonical)
    with kc:
        m = _check(kmc, kc, table, canonical, reads)[(1, 0)]
    if k >= 31:
        assert m.stats[0][1] == 100 and m.stats[0][2] in (2, 3) and m.stats[0][3] == m.stats[0][2] - 1
        assert m.stats[2] == [11, 11, 11, 10]                    # the homopolymer: every window a segment of its own


@pytest.mark.parametrize("k", [5, 31, 33, 63])
def test_hairpin(kmc, oracle, k):
    sample, reads = mi.hairpin(k, 400 + k)
    kc, table = _counter(kmc, oracle, sample, k, True)
    with kc:
        m = _check(kmc, kc, table, True, reads)[(1, 0)]
    if k >= 31:
        assert m.stats[0][2] == 2 and m.stats[0][3] == 1 and sorted(s[2] & 1 for s in m.read_segments[0]) == [0, 1]


_CHILD = r"""
import importlib, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
kmc = importlib.import_module("k-mer-count_amd")
bases, offs = kmc.parse_fasta(sys.argv[2])
same = lambda a, b: all(np.array_equal(x, y) for x, y in zip((a.place, a.stats, a.seg_offsets, a.segments, a.support), (b.place, b.stats, b.seg_offsets, b.segments, b.support)))
with kmc.KmerCounter(k=31) as kc:
    kc.add_batch(bases, offs)
    kc.finalize()
    print("step unitigs(1,0)", file=sys.stderr, flush=True)
    u = kc.unitigs(1, 0)
    print("step map(1,0)", file=sys.stderr, flush=True)
    a = kc.map_reads(bases, offs, 1, 0)
    u2 = kc.unitigs(1, 0)
    assert np.array_equal(u.bases, u2.bases) and np.array_equal(u.offsets, u2.offsets) and np.array_equal(u.abund, u2.abund)
    print("step graph(2,0) map(1,0)", file=sys.stderr, flush=True)
    kc.graph(2, 0, adj=False)
    b = kc.map_reads(bases, offs, 1, 0)
    assert same(a, b)
    print("step links(1,0) map(1,0)", file=sys.stderr, flush=True)
    l1 = kc.unitig_links(1, 0)
    c = kc.map_reads(bases, offs, 1, 0)
    assert same(a, c)
    l2 = kc.unitig_links(1, 0)
    assert np.array_equal(l1.to, l2.to) and np.array_equal(l1.offsets, l2.offsets)
    print("step clean map(1,0)", file=sys.stderr, flush=True)
    v = kc.clean_unitigs(1, 0)
    d = kc.map_reads(bases, offs, 1, 0)
    assert same(a, d)
    v2 = kc.clean_unitigs(1, 0)
    assert np.array_equal(v.verdict, v2.verdict)
    print("step end", file=sys.stderr, flush=True)
"""


def test_map_reuses_the_unitigs_and_leaves_them_alone(kmc):
    """What computes, seen through the KMC_UNITIG_TRACE lines of a child process (nothing is timed)"""
    env = dict(os.environ, KMC_UNITIG_TRACE="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, SAMPLE], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    steps, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("step "):
            cur = line[5:]
            steps[cur] = []
        elif line.startswith("kmc_unitigs:") or line.startswith("kmc_unitig_map:"):
            steps[cur].append(line.split(":")[0] + (" reused" if "unitigs_reused 1" in line else ""))
    assert steps["unitigs(1,0)"] == ["kmc_unitigs"]
    assert steps["map(1,0)"] == ["kmc_unitig_map reused"]                        # behind kmc_unitigs of the same range
    assert steps["graph(2,0) map(1,0)"] == ["kmc_unitigs", "kmc_unitig_map"]      # adj was rewritten: it computes them again
    assert steps["links(1,0) map(1,0)"] == ["kmc_unitig_map reused"]
    assert steps["clean map(1,0)"] == ["kmc_unitig_map reused"]
    assert "index_ms" in r.stderr and "place_ms" in r.stderr and "segs_ms" in r.stderr


def test_the_index_and_the_three_gathers_agree(kmc, oracle):
    """KMC_MAP_NO_INDEX: the place kernel built to gather adj, the ranking and uid_of per window gives the same arrays"""
    k = 31
    sample, reads = mi.genome_reads(k, 100 + k)
    code = _CHILD.split("with kmc.KmerCounter")[0] + r"""
with kmc.KmerCounter(k=31) as kc:
    kc.add_batch(bases, offs)
    kc.finalize()
    a = kc.map_reads(bases, offs, 1, 0)
    np.save(sys.argv[3], a.place)
    print(a.summary.words())
"""
    import tempfile
    reads = [s for s in reads if s]                              # (a FASTA file holds no empty record)
    want = _want(mm.map_reads(gm.count_table(reads, k, True), True, reads))[0]
    with tempfile.TemporaryDirectory() as d:
        fa = os.path.join(d, "r.fasta")
        with open(fa, "w") as f:
            f.write("".join(">r%d\n%s\n" % (i, s) for i, s in enumerate(reads)))
        out = []
        for env in ({}, {"KMC_MAP_NO_INDEX": "1"}):
            p = os.path.join(d, "place%d.npy" % len(out))
            r = subprocess.run([sys.executable, "-c", code, ROOT, fa, p], capture_output=True, text=True, env=dict(os.environ, **env))
            assert r.returncode == 0, r.stderr[-2000:]
            out.append((np.load(p), r.stdout))
    assert np.array_equal(out[0][0], want) and np.array_equal(out[1][0], want) and out[0][1] == out[1][1]


def test_empty_inputs_and_errors(kmc, oracle):
    L = kmc.lib()
    k = 31
    sample, reads = mi.genome_reads(k, 5, n_reads=20, genome=600)
    bases, offs = mi.pack(reads)
    w = (C.c_uint64 * 8)(*([7] * 8))
    n1, n2 = C.c_uint64(9), C.c_uint64(9)
    args = lambda b, o, n: (b.ctypes.data, o.ctypes.data, n, None, None, None, None, 0, None, 0, C.byref(n1), C.byref(n2), w)
    with kmc.KmerCounter(k=k) as kc:
        # no view
        assert L.kmc_unitig_map(kc._h, 1, 0, *args(bases, offs, len(reads))) == kmc.ERR_STATE
        assert L.kmc_unitig_map_device(kc._h, 1, 0, None, None, 0, 0, None, None, None, None, None, None, None, None) == kmc.ERR_STATE
        # an empty view: nothing is placed, the valid windows are still counted
        kc.finalize()
        m = mm.ReadMap(reads, k, True, [])
        r = kc.map_reads(bases, offs)
        assert r.summary.words() == m.summary and m.summary[2] == 0 and m.summary[1] > 0 and len(r.support) == 0 and len(r.segments) == 0
        assert (r.place == mm.NONE).all() and np.array_equal(r.stats, np.array(m.stats, U32)) and not r.seg_offsets.any()
    kc, table = _counter(kmc, oracle, sample, k, True)
    with kc:
        # n_reads == 0
        z = np.zeros(1, U64)
        r = kc.map_reads(np.zeros(0, np.uint8), z)
        assert r.summary.words() == [0] * 8 and len(r.place) == 0 and list(r.seg_offsets) == [0] and not r.support.any()
        assert len(r.support) == um.unitigs(table, True).summary[0]
        assert L.kmc_unitig_map(kc._h, 1, 0, None, None, 0, None, None, None, None, 0, None, 0, C.byref(n1), C.byref(n2), w) == 0
        assert (n1.value, n2.value, list(w)) == (0, len(r.support), [0] * 8)
        # arguments
        assert L.kmc_unitig_map(None, 1, 0, *args(bases, offs, len(reads))) == kmc.ERR_ARG
        assert L.kmc_unitig_map(kc._h, 3, 2, *args(bases, offs, len(reads))) == kmc.ERR_ARG
        bad = offs.copy()
        bad[3] = bad[2] - 1
        assert L.kmc_unitig_map(kc._h, 1, 0, *args(bases, bad, len(reads))) == kmc.ERR_ARG
        # caps too small: KMC_ERR_ARG, the counts are set and nothing is written
        m = mm.map_reads(table, True, reads)
        ns, nu = m.summary[3], m.n_unitigs
        assert ns > 1 and nu > 1
        segs, sup, place = np.full(4 * ns, 0xEEEEEEEE, U32), np.full(nu, 0xEEEE, U64), np.full(len(bases), 0xEEEE, U64)
        for cs, cu in ((ns - 1, nu), (ns, nu - 1)):
            rc = L.kmc_unitig_map(kc._h, 1, 0, bases.ctypes.data, offs.ctypes.data, len(reads), place.ctypes.data, None, None, segs.ctypes.data, cs,
                                  sup.ctypes.data, cu, C.byref(n1), C.byref(n2), None)
            assert rc == kmc.ERR_ARG and (n1.value, n2.value) == (ns, nu)
            assert (segs == 0xEEEEEEEE).all() and (sup == 0xEEEE).all() and (place == 0xEEEE).all()
        # ... and an array that is NULL has no cap
        assert L.kmc_unitig_map(kc._h, 1, 0, bases.ctypes.data, offs.ctypes.data, len(reads), None, None, None, None, 0, sup.ctypes.data, nu,
                                C.byref(n1), C.byref(n2), None) == 0
        assert np.array_equal(sup, np.array(m.support, U64))
    with kmc.KmerCounter(mode=kmc.MODE_LR) as lr:
        assert L.kmc_unitig_map(lr._h, 1, 0, *args(bases, offs, len(reads))) == kmc.ERR_ARG
        assert L.kmc_unitig_map_device(lr._h, 1, 0, None, None, 0, 0, None, None, None, None, None, None, None, None) == kmc.ERR_ARG


def _sample_reads(kmc):
    bases, offs = kmc.parse_fasta(SAMPLE)
    return [bases[int(offs[i]):int(offs[i + 1])].tobytes().decode() for i in range(len(offs) - 1)]


@pytest.mark.parametrize("forward", [False, True])
def test_cli_map(kmc, forward):
    k, canonical = 31, not forward
    reads = _sample_reads(kmc)
    table = gm.count_table(reads, k, canonical)
    fw = ["--forward"] if forward else []
    run = lambda *a: subprocess.run([EXE, SAMPLE, "-k", str(k), "--map", SAMPLE] + list(a) + fw, capture_output=True, text=True)
    r = run()
    assert r.returncode == 0 and r.stdout == mm.map_reads(table, canonical, reads).text(), r.stderr
    r = run("--min-count", "2")
    assert r.returncode == 0 and r.stdout == mm.map_reads(table, canonical, reads, 2, 0).text(), r.stderr
    if not forward:
        final = bm.rounds(table, canonical, max_bubble=31, n_rounds=1)[0]
        r = run("--clean", "1", "--bubble-keys", "31")
        assert r.returncode == 0 and r.stdout == mm.map_reads(final, canonical, reads, k=k).text(), r.stderr
