"""GPU checks of kmc_unitig_pairs / kmc_unitig_pairs_device / KmerCounter.pair_links (kmc_pairs.hip.h).  Expected values come
from tests/pair_model.py -- the definitions of include/kmc.h over Python lists, on top of map_model's segments -- applied to
the CPU oracle's table of the same input.  All comparisons are exact, array by array, through every form of the call."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import graph_model as gm
import map_inputs as mi
import pair_inputs as pi
import pair_model as pm
from conftest import ROOT, SAMPLE
from test_map_gpu import _counter, _sample_reads
from test_transits_gpu import _upload
from test_unitig_gpu import _dev_bytes, _dev_u64

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "bin", "k-mer-count")
U64, U32, U8 = np.uint64, np.uint32, np.uint8
KS = (5, 6, 31, 32, 33, 63)
NAMES = ("pair_class", "pair_ends", "pair_value", "rec_ends", "rec_count", "rec_sum", "rec_min", "rec_max", "insert_hist")
BINS = 1024


def _want(p):
    return (np.array(p.pair_class, U8), np.array(p.pair_ends, U32).reshape(-1), np.array(p.pair_value, U64), np.array(p.rec_ends, U32).reshape(-1),
            np.array(p.rec_count, U64), np.array(p.rec_sum, U64), np.array(p.rec_min, U64), np.array(p.rec_max, U64), np.array(p.hist, U64))


def _equal(got, want, ctx, names=NAMES):
    for name, g, w in zip(names, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (ctx, name, g.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g != w)[:5]
        assert not len(bad), (ctx, name, bad, g[bad], w[bad])


def _raw(kmc, kc, lo, hi, bases, offs, n_rec_cap, n_bins=BINS, flags=0, spare=3):
    """kmc_unitig_pairs through ctypes into arrays with `spare` entries more than needed, filled with a pattern"""
    n_pairs = (len(offs) - 1) // 2
    cls, ends, val = np.full(n_pairs + spare, 0xEE, U8), np.full(2 * (n_pairs + spare), 0xEEEE, U32), np.full(n_pairs + spare, 0xEEEE, U64)
    re_ = np.full(2 * (n_rec_cap + spare), 0xEEEE, U32)
    rc, rs, rn, rx = (np.full(n_rec_cap + spare, 0xEEEE, U64) for _ in range(4))
    hist = np.full(n_bins + spare, 0xEEEE, U64)
    n = [C.c_uint64(12345) for _ in range(2)]
    w = (C.c_uint64 * kmc.PAIR_WORDS)()
    kc._chk(kmc.lib().kmc_unitig_pairs(kc._h, lo, hi, n_bins, flags, bases.ctypes.data if len(bases) else None, offs.ctypes.data, len(offs) - 1,
                                       cls.ctypes.data, ends.ctypes.data, val.ctypes.data, n_pairs + spare, re_.ctypes.data, rc.ctypes.data,
                                       rs.ctypes.data, rn.ctypes.data, rx.ctypes.data, n_rec_cap + spare, hist.ctypes.data, n_bins + spare,
                                       *[C.byref(x) for x in n], w))
    assert n[0].value == n_pairs and n[1].value <= n_rec_cap
    nr = n[1].value
    assert (cls[n_pairs:] == 0xEE).all() and (ends[2 * n_pairs:] == 0xEEEE).all() and (val[n_pairs:] == 0xEEEE).all()
    assert (re_[2 * nr:] == 0xEEEE).all() and all((a[nr:] == 0xEEEE).all() for a in (rc, rs, rn, rx)) and (hist[n_bins:] == 0xEEEE).all()
    return (cls[:n_pairs], ends[:2 * n_pairs], val[:n_pairs], re_[:2 * nr], rc[:nr], rs[:nr], rn[:nr], rx[:nr], hist[:n_bins]), list(w)


def _device(kc, lo, hi, bases, offs, n_bins=BINS, accumulate=False):
    """the device form on an uploaded batch, read back"""
    db, do = _upload(bases, offs)
    *p, n_pairs, nr, s = kc.pair_links_device(db.data_ptr(), do.data_ptr(), len(offs) - 1, len(bases), lo, hi, n_bins, accumulate)
    assert all(x % 8 == 0 for x in p[1:])
    u32 = lambda ptr, n: _dev_u64(ptr, (n + 1) // 2).view(U32)[:n].copy()
    return (_dev_bytes(p[0], n_pairs), u32(p[1], 2 * n_pairs), _dev_u64(p[2], n_pairs), u32(p[3], 2 * nr), _dev_u64(p[4], nr), _dev_u64(p[5], nr),
            _dev_u64(p[6], nr), _dev_u64(p[7], nr), _dev_u64(p[8], n_bins)), s.words()


def _check(kmc, kc, table, canonical, reads, ranges=((1, 0), (2, 0)), n_bins=BINS):
    """every form of the call against the model, for every range; returns {range: the model's Pairs}"""
    bases, offs = mi.pack(reads)
    seen = {}
    for lo, hi in ranges:
        p = pm.pairs(table, canonical, [reads], lo, hi, n_bins, k=kc.k)
        want, words = _want(p), p.summary
        ctx = (kc.k, canonical, lo, hi)
        got, w = _raw(kmc, kc, lo, hi, bases, offs, len(reads) // 2, n_bins)
        assert w == words, (ctx, w, words)
        _equal(got, want, ctx + ("host",))
        got, w = _device(kc, lo, hi, bases, offs, n_bins)
        assert w == words, (ctx, w, words)
        _equal(got, want, ctx + ("device",))
        r = kc.pair_links(bases, offs, lo, hi, n_bins)
        _equal((r.pair_class, r.pair_ends.reshape(-1), r.pair_value, r.rec_ends.reshape(-1), r.rec_count, r.rec_sum, r.rec_min, r.rec_max, r.insert_hist),
               want, ctx + ("pair_links",))
        assert r.summary.words() == words and len(r) == words[6] and r.to_text() == p.text(), ctx
        seen[(lo, hi)] = p
    return seen


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", KS)
def test_constructed_libraries(kmc, oracle, k, canonical):
    """library / gap / adjacent / edges / small: every class at every k, the tie rule, the special pairs at the wave and
    workgroup seams"""
    classes = [0] * 5
    for name in ("library", "gap", "adjacent", "edges", "small"):
        sample, pairs = getattr(pi, name)(k, 700 + k, 120) if name == "gap" else getattr(pi, name)(k, 700 + k)
        kc, table = _counter(kmc, oracle, sample, k, canonical)
        with kc:
            p = _check(kmc, kc, table, canonical, pi.reads_of(pairs), ((1, 0), (2, 0)) if name == "library" else ((1, 0),))[(1, 0)]
        classes = [a + b for a, b in zip(classes, p.summary[1:6])]
    # (a forward ctx places no reverse mate: no pair there has o_A != o_B)
    assert all(classes) if canonical else classes[pm.UNPLACED] and classes[pm.SPAN] and classes[pm.SAME_STRAND] and not classes[pm.PROPER] and not classes[pm.EVERTED], classes


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", KS)
def test_inputs_of_the_map_tests(kmc, oracle, k, canonical):
    """the reads of the map tests taken two at a time: gaps, N, short and empty mates, a cycle, a hairpin"""
    inputs = [mi.genome_reads(k, 100 + k), mi.circular(k, 200 + k)]
    if canonical and k % 2 == 1:
        inputs.append(mi.hairpin(k, 400 + k))
    for sample, reads in inputs:
        reads = reads[:len(reads) // 2 * 2]
        kc, table = _counter(kmc, oracle, sample, k, canonical)
        with kc:
            _check(kmc, kc, table, canonical, reads, ((1, 0),))


_HOT_CHILD = r"""
import importlib, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
kmc = importlib.import_module("k-mer-count_amd")
import map_inputs as mi, pair_inputs as pi
sample, pairs = pi.hot(31, 730, 1000)
with kmc.KmerCounter(k=31) as kc:
    kc.add_batch(*mi.pack(sample))
    kc.finalize()
    r = kc.pair_links(*mi.pack(pi.reads_of(pairs)))
    print(r.to_text(), end="")
    print(r.summary.words())
"""


def test_hot_record_counts_exactly(kmc, oracle):
    """1000 pairs on one record: every lane of four workgroups adds to the same three words.  Exact count / sum / min / max,
    with the LDS table and, in a child process, with KMC_PAIRS_PLAIN"""
    k = 31
    sample, pairs = pi.hot(k, 730, 1000)
    kc, table = _counter(kmc, oracle, sample, k, True)
    p = pm.pairs(table, True, [pi.reads_of(pairs)])
    values = [x.frag - 50 for x in pairs]
    assert p.summary == [1000, 0, 1000, 0, 0, 0, 1, 0] and (p.rec_count, p.rec_sum, p.rec_min, p.rec_max) == ([1000], [sum(values)], [min(values)], [max(values)])
    with kc:
        got, w = _device(kc, 1, 0, *mi.pack(pi.reads_of(pairs)))
        assert w == p.summary
        _equal(got, _want(p), "hot")
    want = p.text() + str(p.summary) + "\n"
    for plain in (False, True):
        env = dict(os.environ)
        env.pop("KMC_PAIRS_PLAIN", None)
        if plain:
            env["KMC_PAIRS_PLAIN"] = "1"
        r = subprocess.run([sys.executable, "-c", _HOT_CHILD, ROOT], capture_output=True, text=True, env=env)
        assert r.returncode == 0 and r.stdout == want, (plain, r.stdout[-500:], r.stderr[-2000:])


def test_more_records_than_a_sort_leaf(kmc, oracle):
    k = 31
    sample, pairs = pi.many_records(k, 750)
    kc, table = _counter(kmc, oracle, sample, k, True)
    reads = pi.reads_of(pairs)
    p = pm.pairs(table, True, [reads])
    assert p.summary[6] > 2048, p.summary                      # KMC_MSD_LEAF1
    with kc:
        got, w = _device(kc, 1, 0, *mi.pack(reads))
        assert w == p.summary
        _equal(got, _want(p), "many")
        # ... and added in two halves: the held records go through the sort as weighted keys
        half = len(reads) // 4 * 2
        _device(kc, 1, 0, *mi.pack(reads[:half]))
        got, w = _device(kc, 1, 0, *mi.pack(reads[half:]), accumulate=True)
        assert w == p.summary
        _equal(got[3:], _want(p)[3:], "many, two halves", NAMES[3:])


def test_one_workgroup_takes_every_round_and_overflows_its_table(kmc, oracle):
    """KMC_PAIRS_GRID=1: one workgroup walks the whole batch in two dozen rounds, and its LDS table of 512 slots meets more
    than 2048 distinct records -- the grid-stride loops of the pair and reduce kernels and the fallback behind four failed
    probes, with several leaders per wave, both forced; under ACCUMULATE the held records take the same road"""
    k = 31
    sample, pairs = pi.many_records(k, 750)
    kc, table = _counter(kmc, oracle, sample, k, True)
    reads = pi.reads_of(pairs)
    p = pm.pairs(table, True, [reads])
    assert p.summary[6] > 4 * 512 and len(pairs) > 16 * 256
    os.environ["KMC_PAIRS_GRID"] = "1"
    try:
        with kc:
            got, w = _device(kc, 1, 0, *mi.pack(reads))
            assert w == p.summary
            _equal(got, _want(p), "one workgroup")
            half = len(reads) // 4 * 2
            _device(kc, 1, 0, *mi.pack(reads[:half]))
            got, w = _device(kc, 1, 0, *mi.pack(reads[half:]), accumulate=True)
            assert w == p.summary
            _equal(got[3:], _want(p)[3:], "one workgroup, two halves", NAMES[3:])
    finally:
        os.environ.pop("KMC_PAIRS_GRID", None)


def test_accumulate(kmc, oracle):
    k = 31
    L = kmc.lib()
    sample, pairs = pi.library(k, 700 + k)
    reads = pi.reads_of(pairs)
    kc, table = _counter(kmc, oracle, sample, k, True)
    whole = pm.pairs(table, True, [reads])
    parts = [reads[:74], reads[74:76], [], reads[76:]]                          # three uneven batches and one without a read
    packed = [mi.pack(x) for x in parts]
    none = lambda flags, bins=BINS, lo=1: L.kmc_unitig_pairs_device(kc._h, lo, 0, bins, flags, None, None, 0, 0, *([None] * 12))
    with kc:
        assert none(kmc.PAIR_ACCUMULATE) == kmc.ERR_STATE and "ACCUMULATE" in L.kmc_last_error(kc._h).decode()          # nothing held yet
        got, w = _device(kc, 1, 0, *packed[0])
        first = pm.pairs(table, True, [parts[0]])
        _equal(got, _want(first), "first")
        assert w == first.summary
        for i in (1, 2):
            got, w = _device(kc, 1, 0, *packed[i], accumulate=True)
            so_far = pm.pairs(table, True, parts[:i + 1])
            _equal(got, _want(so_far), ("batch", i))
            assert w == so_far.summary
        # a map, a transits and a profile call in between do not disturb the totals; another n_bins or range has nothing held
        kc.map_reads(*mi.pack(reads))
        kc.transits(*mi.pack(reads))
        kc.profile(*mi.pack(reads))
        assert none(kmc.PAIR_ACCUMULATE, BINS - 1) == kmc.ERR_STATE and none(kmc.PAIR_ACCUMULATE, BINS, 2) == kmc.ERR_STATE
        got, w = _raw(kmc, kc, 1, 0, *packed[3], len(reads) // 2, flags=kmc.PAIR_ACCUMULATE)      # the last through the host form
        acc = pm.pairs(table, True, parts)
        assert acc.totals() == whole.totals()
        _equal(got, _want(acc), "whole")
        assert w == whole.summary
        # n_reads == 0 with the flag returns the held result; without it a call replaces what is held
        assert none(kmc.PAIR_ACCUMULATE) == 0
        got, w = _device(kc, 1, 0, *packed[2], accumulate=True)
        _equal(got[3:], _want(whole)[3:], "held", NAMES[3:])
        assert w == whole.summary and len(got[0]) == 0
        got, w = _device(kc, 1, 0, *packed[1])
        _equal(got, _want(pm.pairs(table, True, [parts[1]])), "replaced")
        # a kmc_graph call of another range drops what is held (the next call computes the unitigs again); so does a finalize
        assert none(kmc.PAIR_ACCUMULATE) == 0
        kc.graph(2, 0, adj=False)
        assert none(kmc.PAIR_ACCUMULATE) == kmc.ERR_STATE
        assert none(0) == 0 and none(kmc.PAIR_ACCUMULATE) == 0
        kc.add_batch(*mi.pack(sample))
        kc.finalize()
        assert none(kmc.PAIR_ACCUMULATE) == kmc.ERR_STATE


def test_a_finalize_with_nothing_added_keeps_the_held_result(kmc, oracle):
    k = 31
    sample, pairs = pi.adjacent(k, 720 + k)
    reads = pi.reads_of(pairs)
    kc, table = _counter(kmc, oracle, sample, k, True)
    twice = pm.pairs(table, True, [reads, reads])
    with kc:
        _device(kc, 1, 0, *mi.pack(reads))
        view = kc.export_device()
        assert kc.finalize() == (len(table), sum(table.values())) and kc.export_device() == view
        got, w = _device(kc, 1, 0, *mi.pack(reads), accumulate=True)
        _equal(got, _want(twice), "behind a finalize with nothing added")
        assert w == twice.summary


_CHILD = r"""
import importlib, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
kmc = importlib.import_module("k-mer-count_amd")
bases, offs = kmc.parse_fasta(sys.argv[2])
arrays = lambda p: (p.pair_class, p.pair_ends, p.pair_value, p.rec_ends, p.rec_count, p.rec_sum, p.rec_min, p.rec_max, p.insert_hist)
same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(arrays(a), arrays(b))) and a.summary == b.summary
with kmc.KmerCounter(k=31) as kc:
    kc.add_batch(bases, offs)
    kc.finalize()
    before = kc.export()
    print("step transits pairs contigs", file=sys.stderr, flush=True)
    t = kc.transits(bases, offs, 1, 0)
    a = kc.pair_links(bases, offs, 1, 0)
    assert a.summary.pairs == (len(offs) - 1) // 2 and a.summary.span > 0
    c = kc.contigs(1, 0)
    assert c.summary.contigs > 0
    print("step pairs transits pairs", file=sys.stderr, flush=True)
    from importlib import import_module
    view = import_module("k-mer-count_amd.distributed").device_view
    d = kc.pair_links_device(0, 0, 0, 0, 1, 0, 1024, True)       # the held result: its pointers ...
    read = lambda: [view(d[i], d[10], "cuda:0").cpu().numpy().view(np.uint64).copy() for i in (4, 5, 6, 7)]
    held = read()
    assert all(np.array_equal(x, y) for x, y in zip(held, (a.rec_count, a.rec_sum, a.rec_min, a.rec_max))) and d[10] == len(a) > 0
    t2 = kc.transits(bases, offs, 1, 0)
    assert all(np.array_equal(x, y) for x, y in zip(held, read()))        # ... read again behind a transits call
    assert kc.pair_links_device(0, 0, 0, 0, 1, 0, 1024, True) == d and np.array_equal(t.link_support, t2.link_support)
    print("step graph(2,0) pairs(1,0)", file=sys.stderr, flush=True)
    kc.graph(2, 0, adj=False)
    b = kc.pair_links(bases, offs, 1, 0)
    assert same(a, b)
    print("step pairs(1,0) again", file=sys.stderr, flush=True)
    assert same(a, kc.pair_links(bases, offs, 1, 0))
    assert kc.export().equals(before)
    print("step end", file=sys.stderr, flush=True)
"""


def test_orderings_through_the_trace_lines(kmc):
    """What computes, seen through the KMC_UNITIG_TRACE lines of a child process (nothing is timed); the view is exported
    before and after and must be the same table"""
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
            steps[cur].append(name + (" reused" if name == "kmc_unitig_pairs" and "unitigs_reused 1" in line else ""))
    assert steps["transits pairs contigs"] == ["kmc_unitigs", "kmc_unitig_links", "kmc_unitig_map", "kmc_unitig_transits", "kmc_unitig_map",
                                               "kmc_unitig_pairs reused", "kmc_unitig_contigs"]
    assert steps["pairs transits pairs"] == ["kmc_unitig_map", "kmc_unitig_transits"]       # (a pairs call that adds no read computes nothing)
    assert steps["graph(2,0) pairs(1,0)"] == ["kmc_unitigs", "kmc_unitig_map", "kmc_unitig_pairs"]
    assert steps["pairs(1,0) again"] == ["kmc_unitig_map", "kmc_unitig_pairs reused"]
    line = [x for x in r.stderr.splitlines() if x.startswith("kmc_unitig_pairs:")][0].split()
    assert line[1:12:2] == ["unitigs", "pairs", "span", "proper", "records", "unitigs_reused"]
    assert line[13::2] == ["map_ms", "anchor_ms", "sort_ms", "reduce_ms"]


def test_export_is_byte_identical_around_a_pairs_call(kmc, oracle):
    """the sort of the records touched nothing of the view: kmc_export before and after, byte for byte"""
    k = 31
    sample, pairs = pi.many_records(k, 750, genome=6000, n_pairs=600)
    kc, table = _counter(kmc, oracle, sample, k, True)
    with kc:
        kc.finalize()
        before = kc.export()
        r = kc.pair_links(*mi.pack(pi.reads_of(pairs)))
        assert r.summary.records > 100
        after = kc.export()
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip((before.key_hi, before.key_lo, before.count), (after.key_hi, after.key_lo, after.count)))


def test_empty_inputs_and_errors(kmc, oracle):
    L = kmc.lib()
    k = 31
    sample, pairs = pi.adjacent(k, 720 + k, n_pairs=20)
    reads = pi.reads_of(pairs)
    bases, offs = mi.pack(reads)
    n = [C.c_uint64(9) for _ in range(2)]
    w = (C.c_uint64 * 8)(*([7] * 8))
    tail = lambda: [C.byref(x) for x in n] + [w]
    plain = lambda h, lo, hi, bins, flags, b, o, nr: L.kmc_unitig_pairs(h, lo, hi, bins, flags, b.ctypes.data, o.ctypes.data, nr, None, None, None, 0,
                                                                        None, None, None, None, None, 0, None, 0, *tail())
    dev_none = lambda h: L.kmc_unitig_pairs_device(h, 1, 0, BINS, 0, None, None, 0, 0, *([None] * 12))
    with kmc.KmerCounter(k=k) as kc:
        assert plain(kc._h, 1, 0, BINS, 0, bases, offs, len(reads)) == kmc.ERR_STATE and dev_none(kc._h) == kmc.ERR_STATE      # no view
        kc.finalize()                                                                                                       # an empty view
        r = kc.pair_links(bases, offs)
        assert r.summary.words() == [len(pairs), len(pairs), 0, 0, 0, 0, 0, 0] and not r.pair_class.any() and (r.pair_ends == kmc.MAP_NONE).all()
        assert not r.pair_value.any() and len(r) == 0 and not r.insert_hist.any() and r.to_text() == ""
    kc, table = _counter(kmc, oracle, sample, k, True)
    p = pm.pairs(table, True, [reads])
    with kc:
        # no reads: zeros; two reads: one pair
        r = kc.pair_links(np.zeros(0, U8), np.zeros(1, U64))
        assert r.summary.words() == [0] * 8 and len(r.pair_class) == 0 and len(r) == 0 and not r.insert_hist.any()
        assert plain(kc._h, 1, 0, BINS, 0, bases, offs, 0) == 0 and [x.value for x in n] == [0, 0] and list(w) == [0] * 8
        one = pm.pairs(table, True, [reads[:2]])
        got, words = _raw(kmc, kc, 1, 0, *mi.pack(reads[:2]), 1)
        _equal(got, _want(one), "one pair")
        assert words == one.summary == [1, 0, 1, 0, 0, 0, 1, 0]
        # arguments
        assert plain(None, 1, 0, BINS, 0, bases, offs, len(reads)) == kmc.ERR_ARG
        assert plain(kc._h, 3, 2, BINS, 0, bases, offs, len(reads)) == kmc.ERR_ARG
        assert plain(kc._h, 1, 0, BINS, 0, bases, offs, len(reads) - 1) == kmc.ERR_ARG and "pairs" in L.kmc_last_error(kc._h).decode()       # odd
        assert plain(kc._h, 1, 0, BINS, 2, bases, offs, len(reads)) == kmc.ERR_ARG and "flag" in L.kmc_last_error(kc._h).decode()
        assert plain(kc._h, 1, 0, BINS, 0x80000001, bases, offs, len(reads)) == kmc.ERR_ARG
        for bins in (0, 1, (1 << 20) + 1):
            assert plain(kc._h, 1, 0, bins, 0, bases, offs, len(reads)) == kmc.ERR_ARG and "n_bins" in L.kmc_last_error(kc._h).decode()
        assert plain(kc._h, 1, 0, 2, 0, bases, offs, len(reads)) == 0 and plain(kc._h, 1, 0, 1 << 20, 0, bases, offs, len(reads)) == 0
        bad = offs.copy()
        bad[3] = bad[2] - 1
        assert plain(kc._h, 1, 0, BINS, 0, bases, bad, len(reads)) == kmc.ERR_ARG
        # every cap one too small: KMC_ERR_ARG, the sizes are set and nothing is written
        npair, nr = len(pairs), p.summary[6]
        assert nr == 1
        cls, val, rc_, hist = np.full(npair, 0xEE, U8), np.full(npair, 0xEEEE, U64), np.full(nr, 0xEEEE, U64), np.full(BINS, 0xEEEE, U64)
        for cp, cr, cb in ((npair - 1, nr, BINS), (npair, nr - 1, BINS), (npair, nr, BINS - 1)):
            rc = L.kmc_unitig_pairs(kc._h, 1, 0, BINS, 0, bases.ctypes.data, offs.ctypes.data, len(reads), cls.ctypes.data, None, val.ctypes.data, cp,
                                    None, rc_.ctypes.data, None, None, None, cr, hist.ctypes.data, cb, *tail())
            assert rc == kmc.ERR_ARG and [x.value for x in n] == [npair, nr], (cp, cr, cb, rc)
            assert (cls == 0xEE).all() and (val == 0xEEEE).all() and (rc_ == 0xEEEE).all() and (hist == 0xEEEE).all()
        # ... and an array that is NULL has no cap
        assert L.kmc_unitig_pairs(kc._h, 1, 0, BINS, 0, bases.ctypes.data, offs.ctypes.data, len(reads), None, None, None, 0, None, rc_.ctypes.data,
                                  None, None, None, nr, None, 0, *tail()) == 0
        assert list(rc_) == p.rec_count and list(w) == p.summary
    with kmc.KmerCounter(mode=kmc.MODE_LR) as lr:
        assert plain(lr._h, 1, 0, BINS, 0, bases, offs, len(reads)) == kmc.ERR_ARG and dev_none(lr._h) == kmc.ERR_ARG


@pytest.mark.parametrize("forward", [False, True])
def test_cli_pairs(kmc, forward, tmp_path):
    k, canonical = 31, not forward
    sample, pairs = pi.library(k, 700 + k)
    ref, mates = tmp_path / "ref.fa", tmp_path / "mates.fa"
    ref.write_text("".join(">s%d\n%s\n" % (i, s) for i, s in enumerate(sample)))
    reads = pi.reads_of(pairs)
    mates.write_text("".join(">r%d/%d\n%s\n" % (i // 2, i % 2 + 1, s) for i, s in enumerate(reads)))
    table = gm.count_table(sample, k, canonical)
    fw = ["--forward"] if forward else []
    run = lambda *a: subprocess.run([EXE, str(ref), "-k", str(k), "--pairs", str(mates)] + list(a) + fw, capture_output=True, text=True)
    r = run()
    want = pm.pairs(table, canonical, [reads])
    assert r.returncode == 0 and r.stdout == want.text() and r.stdout.count("P\t") > 0, r.stderr
    r = run("--insert-bins", "200", "--min-count", "2")
    assert r.returncode == 0 and r.stdout == pm.pairs(table, canonical, [reads], 2, 0, 200).text(), r.stderr
