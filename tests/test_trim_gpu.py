"""GPU checks of kmc_trim / kmc_trim_device / KmerCounter.trim_reads (kmc_trim.hip.h).  Expected values come from
tests/trim_model.py -- the definitions of include/kmc.h on Python strings -- applied to the CPU oracle's table of the same
input.  All comparisons are exact, entry by entry, through every form of the call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bubble_model as bm
import correct_model as cm
import graph_model as gm
import trim_inputs as ti
import trim_model as tm
from conftest import ROOT, SAMPLE
from test_correct_gpu import _counter, _sample_reads, _upload
from test_unitig_gpu import _dev_bytes, _dev_u64

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "bin", "k-mer-count")
U64, U32, U8 = np.uint64, np.uint32, np.uint8
RANGES = ((1, 0), (2, 0), (2, 3))
MODES = (dict(mode=tm.NONE), dict(mode=tm.ENDS), dict(mode=tm.LONGEST))
NAMES = ("bases", "offsets", "origin", "stats", "verdict")
# the reduce kernel's variants, in windows (kmc_trim.hip.h: "#define KMC_TR_LANE_MAX 1024u", "#define KMC_TR_WAVE_MAX 32768u")
LANE_MAX, WAVE_MAX = 1024, 32768


def _rule(mode=tm.LONGEST, flags=0, min_strong=0, min_permille=0, min_len=0):
    return mode, flags, min_strong, min_permille, min_len


def _want(m):
    return (np.frombuffer("".join(m.out).encode(), U8), np.array(m.offsets, U64), np.array(m.origin, U64),
            np.array(m.stats, U32).reshape(-1, 4), np.array(m.verdict, U8))


def _equal(got, want, ctx):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.size == w.size, (ctx, name, g.dtype, g.shape, w.shape)
        g = g.reshape(w.shape)
        bad = np.flatnonzero((g != w).reshape(len(w), -1).any(axis=1))[:5] if w.size else []
        assert not len(bad), (ctx, name, bad, g[bad], w[bad])


def _raw(kmc, kc, lo, hi, rule, bases, offs, no, nb, spare=3):
    """kmc_trim through ctypes into arrays with `spare` entries more than needed, filled with a pattern"""
    L = kmc.lib()
    nr = len(offs) - 1
    out, oo, org = np.full(nb + spare, 0xEE, U8), np.full(no + 1 + spare, 0xEEEE, U64), np.full(no + spare, 0xEEEE, U64)
    stats, verdict = np.full(4 * nr + spare, 0xEEEEEEEE, U32), np.full(nr + spare, 0xEE, U8)
    n1, n2 = C.c_uint64(12345), C.c_uint64(12345)
    w = (C.c_uint64 * kmc.TRIM_WORDS)()
    kc._chk(L.kmc_trim(kc._h, lo, hi, *rule, bases.ctypes.data, offs.ctypes.data, nr, out.ctypes.data, nb + spare, oo.ctypes.data, org.ctypes.data,
                       no + spare, stats.ctypes.data, verdict.ctypes.data, C.byref(n1), C.byref(n2), w))
    assert (n1.value, n2.value) == (no, nb)
    assert (out[nb:] == 0xEE).all() and (oo[no + 1:] == 0xEEEE).all() and (org[no:] == 0xEEEE).all()
    assert (stats[4 * nr:] == 0xEEEEEEEE).all() and (verdict[nr:] == 0xEE).all()
    return (out[:nb], oo[:no + 1], org[:no], stats[:4 * nr], verdict[:nr]), list(w)


def _read_back(p, no, nb, nr):
    db, doo, dorg, ds, dv = p
    assert db % 16 == 0 and doo % 8 == 0 and dorg % 8 == 0 and ds % 16 == 0
    padded = _dev_bytes(db, (nb + 15) // 16 * 16)
    assert not padded[nb:].any()                     # zero up to the 16-byte boundary
    return padded[:nb], _dev_u64(doo, no + 1), _dev_u64(dorg, no), _dev_bytes(ds, 16 * nr).view(U32), _dev_bytes(dv, nr)


def _device(kc, lo, hi, rule, bases, offs):
    """the device form on an uploaded batch, read back"""
    nr, nb = len(offs) - 1, len(bases)
    db, do = _upload(bases, offs)
    *p, no, nob, s = kc.trim_reads_device(db.data_ptr(), do.data_ptr(), nr, nb, lo, hi, *rule)
    return _read_back(p, no, nob, nr), no, nob, s.words()


def _check(kmc, kc, table, canonical, reads, ranges=RANGES, rules=MODES):
    """every form of the call against the model, for every range and rule; returns {(range, rule number): the model's result}"""
    L = kmc.lib()
    bases, offs = ti.pack(reads)
    seen = {}
    for lo, hi in ranges:
        words = None
        for ri, kw in enumerate(rules):
            m = tm.trim_reads(table, canonical, reads, lo, hi, k=kc.k, words=words, **kw)
            words = m.words
            rule = _rule(**kw)
            want, summary = _want(m), m.summary
            no, nb = summary[4], summary[5]
            ctx = (kc.k, canonical, lo, hi, rule)
            # the sizing call
            n1, n2 = C.c_uint64(1), C.c_uint64(1)
            w = (C.c_uint64 * 8)()
            kc._chk(L.kmc_trim(kc._h, lo, hi, *rule, bases.ctypes.data, offs.ctypes.data, len(reads), None, 0, None, None, 0, None, None,
                               C.byref(n1), C.byref(n2), w))
            assert (n1.value, n2.value, list(w)) == (no, nb, summary), (ctx, n1.value, n2.value, list(w), summary)
            got, w = _raw(kmc, kc, lo, hi, rule, bases, offs, no, nb)
            assert w == summary, (ctx, w, summary)
            _equal(got, want, ctx + ("host",))
            got, dno, dnb, w = _device(kc, lo, hi, rule, bases, offs)
            assert (dno, dnb, w) == (no, nb, summary), (ctx, dno, dnb, w, summary)
            _equal(got, want, ctx + ("device",))
            r = kc.trim_reads(bases, offs, lo, hi, *rule)
            _equal((r.bases, r.offsets, r.origin, r.stats, r.verdict), want, ctx + ("trim_reads",))
            assert r.summary.words() == summary and len(r) == no and r.strings() == m.out and r.to_fasta() == m.text()
            seen[((lo, hi), ri)] = m
    return seen


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [5, 6, 31, 32, 33, 63])
def test_key_widths_strands_and_gaps(kmc, oracle, k, canonical):
    """key widths and parities; both strands; N inside, lower case, reads of k - 1, k and k + 1 bases, empty reads, a read of
    N only; all three ranges and modes"""
    sample, reads = ti.genome_reads(k, 100 + k)
    kc, table = _counter(kmc, oracle, sample, k, canonical)
    with kc:
        seen = _check(kmc, kc, table, canonical, reads)
        if k >= 31:     # (at k = 5 and 6 the sample fills the k-mer space: those check exactness alone)
            m = seen[((2, 0), 2)]
            assert m.summary[6] >= 30 and 0 < m.summary[4] < len(reads) and m.summary[7] > m.summary[5]
            # words [0], [1] against kmc_correct's and kmc_profile's per-read words
            bases, offs = ti.pack(reads)
            c = kc.correct_reads(bases, offs, 2, 3)
            t = kc.trim_reads(bases, offs, 2, 3, tm.NONE)
            assert np.array_equal(t.stats[:, 0], c.stats[:, 0]) and np.array_equal(t.stats[:, 1], c.stats[:, 0] - c.stats[:, 1])
            _, ps = kc.profile(bases, offs, min_count=2, windows=False)
            t = kc.trim_reads(bases, offs, 2, 0, tm.NONE)
            assert np.array_equal(t.stats[:, :2].astype(U64), ps[:, :2])


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [31, 32])
def test_run_shapes_by_name(kmc, oracle, k, canonical):
    sample, reads, names, d = ti.shapes(k, 40 + k)
    kc, table = _counter(kmc, oracle, sample, k, canonical)
    bases, offs = ti.pack(reads)
    with kc:
        _check(kmc, kc, table, canonical, reads, ((2, 0),))
        ends, longest = kc.trim_reads(bases, offs, 2, 0, tm.ENDS), kc.trim_reads(bases, offs, 2, 0, tm.LONGEST)
    row = lambda r, name: r.stats[names[name]].tolist()
    L = lambda name: len(reads[names[name]])
    assert row(longest, "all_strong") == [d - 1, d - 1, 0, L("all_strong")] and row(longest, "none_strong") == [d - 1, 0, 0, 0]
    assert row(longest, "weak_at_0") == [d, d - 1, 1, L("weak_at_0") - 1] and row(longest, "weak_at_last") == [d, d - 1, 0, L("weak_at_last") - 1]
    assert row(longest, "weak_in_the_middle") == [2 * d - 1, 2 * d - 2, 0, d + k - 2]        # two longest runs: the first wins
    assert row(longest, "longest_run_last") == [d + 5, d + 4, 6, d + k - 2]
    assert row(ends, "weak_in_the_middle") == [2 * d - 1, 2 * d - 2, 0, L("weak_in_the_middle")]
    q = L("split_by_N") // 2
    assert row(ends, "split_by_N") == [d - 1 - k, d - 1 - k, 0, L("split_by_N")] and row(longest, "split_by_N")[3] == max(q, L("split_by_N") - q - 1)
    assert row(ends, "ends_with_weak_inside") == [L("ends_with_weak_inside") - k + 1, L("ends_with_weak_inside") - k - 2, 0, L("ends_with_weak_inside")]
    assert names["none_strong"] not in longest.origin.tolist() and len(longest) == len(reads) - 1


@pytest.mark.parametrize("canonical", [True, False])
def test_word_and_chunk_seams(kmc, oracle, canonical):
    k = 31
    sample, reads = ti.seams(k, 7)
    kc, table = _counter(kmc, oracle, sample, k, canonical)
    with kc:
        m = _check(kmc, kc, table, canonical, reads, ((1, 0),))[((1, 0), 2)]
    assert m.stats[0][:2] == [2970, 2970 - len(ti.SEAM_WEAK_ENDS)] and sum(map(len, reads[:2])) == 3072
    sample, reads = ti.starts_at_1024(k, 8)
    assert len(reads[0]) == 1024
    kc, table = _counter(kmc, oracle, sample, k, canonical)
    with kc:
        m = _check(kmc, kc, table, canonical, reads, ((2, 0),))[((2, 0), 2)]
    assert m.summary[4] == 4 and m.summary[6] == 4


@pytest.mark.parametrize("canonical", [True, False])
def test_reduce_variant_boundaries(kmc, oracle, canonical):
    """reads of exactly LANE_MAX and WAVE_MAX windows, one fewer and one more; the longest run across two lanes' slices (5000
    bases, a wave) and across two waves' (70 000 bases, a workgroup)"""
    k = 31
    sample, reads = ti.variants(k, 9)
    assert [len(r) - k + 1 for r in reads[:6]] == [LANE_MAX - 1, LANE_MAX, LANE_MAX + 1, WAVE_MAX - 1, WAVE_MAX, WAVE_MAX + 1]
    kc, table = _counter(kmc, oracle, sample, k, canonical)
    with kc:
        m = _check(kmc, kc, table, canonical, reads, ((1, 0),))[((1, 0), 2)]
    assert m.stats[6][2:] == [701, 1900 - 701] and m.stats[7][2:] == [18001, 22500 - 18001]


@pytest.mark.parametrize("canonical", [True, False])
def test_many_short_reads(kmc, oracle, canonical):
    k = 31
    sample, reads = ti.many_short(k, 10)
    kc, table = _counter(kmc, oracle, sample, k, canonical)
    with kc:
        m = _check(kmc, kc, table, canonical, reads, ((2, 0),))[((2, 0), 2)]
    assert len(reads) == 3000 and m.summary[4] >= 2900 and m.summary[6] >= 2900


def test_gather_alignment(kmc, oracle):
    """spans of 0, 1, 15, 16, 17, 31, 32 and 33 bases from every source alignment to every destination alignment; sixteen
    reads and empty emitted reads in one 16-byte block"""
    k = 31
    sample, reads, met = ti.alignment(k, 11)
    assert len(met) == 8 * 256
    kc, table = _counter(kmc, oracle, sample, k, True)
    with kc:
        seen = _check(kmc, kc, table, True, reads, ((2, 0),),
                      (dict(mode=tm.NONE, flags=tm.INVERT, min_strong=1), dict(mode=tm.NONE), dict(mode=tm.LONGEST), dict(mode=tm.NONE, min_strong=1)))
    m = seen[((2, 0), 0)]
    assert m.summary[4] == len(reads) - 8 * 256 and sum(1 for s in m.out if not s) >= 5


def test_flags_and_argument_errors(kmc, oracle):
    k = 31
    L = kmc.lib()
    sample, reads = ti.pairs(k, 3)
    kc, table = _counter(kmc, oracle, sample, k, True)
    bases, offs = ti.pack(reads)
    n1, n2 = C.c_uint64(9), C.c_uint64(9)
    call = lambda h, lo, hi, rule, n: L.kmc_trim(h, lo, hi, *rule, bases.ctypes.data, offs.ctypes.data, n, None, 0, None, None, 0, None, None,
                                                 C.byref(n1), C.byref(n2), None)
    with kc:
        rules = [dict(mode=tm.NONE, min_strong=1, flags=f) for f in (0, tm.INVERT, tm.PAIR_BOTH, tm.PAIR_EITHER, tm.INVERT | tm.PAIR_BOTH, tm.INVERT | tm.PAIR_EITHER)]
        rules += [dict(mode=tm.LONGEST, flags=tm.PAIR_BOTH), dict(mode=tm.ENDS, flags=tm.PAIR_EITHER, min_strong=1)]
        seen = _check(kmc, kc, table, True, reads, ((2, 0),), rules)
        em = lambda i: [bool(v & tm.EMITTED) for v in seen[((2, 0), i)].verdict]
        assert em(0) == [True, True, True, False, False, True, False, False] * 2 and em(1) == [not x for x in em(0)]
        assert em(2) == ([True] * 2 + [False] * 6) * 2 and em(3) == ([True] * 6 + [False] * 2) * 2
        # each argument error by name
        assert call(kc._h, 1, 0, _rule(tm.NONE, tm.PAIR_BOTH), len(reads) - 1) == kmc.ERR_ARG          # odd n_reads with a pair flag
        assert call(kc._h, 1, 0, _rule(tm.NONE, tm.PAIR_BOTH | tm.PAIR_EITHER), len(reads)) == kmc.ERR_ARG
        assert call(kc._h, 1, 0, _rule(tm.LONGEST, tm.INVERT), len(reads)) == kmc.ERR_ARG              # INVERT with trimming
        assert call(kc._h, 1, 0, _rule(tm.ENDS, tm.INVERT), len(reads)) == kmc.ERR_ARG
        assert call(kc._h, 1, 0, _rule(tm.NONE, min_permille=1001), len(reads)) == kmc.ERR_ARG
        assert call(kc._h, 1, 0, _rule(3), len(reads)) == kmc.ERR_ARG and call(kc._h, 1, 0, _rule(-1), len(reads)) == kmc.ERR_ARG    # unknown mode
        assert call(kc._h, 1, 0, _rule(tm.NONE, 8), len(reads)) == kmc.ERR_ARG                         # unknown flag bit
        assert call(kc._h, 3, 2, _rule(), len(reads)) == kmc.ERR_ARG                                   # max below min
        assert call(None, 1, 0, _rule(), len(reads)) == kmc.ERR_ARG and (n1.value, n2.value) == (0, 0)
        bad = offs.copy()
        bad[3] = bad[2] - 1
        assert L.kmc_trim(kc._h, 1, 0, *_rule(), bases.ctypes.data, bad.ctypes.data, len(reads), None, 0, None, None, 0, None, None,
                          C.byref(n1), C.byref(n2), None) == kmc.ERR_ARG
        assert call(kc._h, 1, 0, _rule(), len(reads)) == 0
        # a cap one too small: KMC_ERR_ARG, the counts are set and nothing is copied; an array that is NULL has no cap
        m = seen[((2, 0), 0)]
        no, nb = m.summary[4], m.summary[5]
        out, oo, org = np.full(nb, 0xEE, U8), np.full(no + 1, 0xEEEE, U64), np.full(no, 0xEEEE, U64)
        host = lambda o, cb, a, b, cr: L.kmc_trim(kc._h, 2, 0, *_rule(tm.NONE, 0, 1), bases.ctypes.data, offs.ctypes.data, len(reads), o, cb, a, b, cr,
                                                  None, None, C.byref(n1), C.byref(n2), None)
        assert host(out.ctypes.data, nb - 1, oo.ctypes.data, org.ctypes.data, no) == kmc.ERR_ARG and (n1.value, n2.value) == (no, nb)
        assert host(out.ctypes.data, nb, oo.ctypes.data, org.ctypes.data, no - 1) == kmc.ERR_ARG
        assert (out == 0xEE).all() and (oo == 0xEEEE).all() and (org == 0xEEEE).all()
        assert host(out.ctypes.data, nb, None, None, 0) == 0 and out.tobytes().decode() == "".join(m.out)
    with kmc.KmerCounter(k=k) as fresh:
        assert call(fresh._h, 1, 0, _rule(), len(reads)) == kmc.ERR_STATE                              # no view
        assert L.kmc_trim_device(fresh._h, 1, 0, *_rule(), None, None, 0, 0, None, None, None, None, None, None, None, None) == kmc.ERR_STATE
    with kmc.KmerCounter(mode=kmc.MODE_LR) as lr:
        assert call(lr._h, 1, 0, _rule(), len(reads)) == kmc.ERR_ARG                                   # LR ctx
        assert L.kmc_trim_device(lr._h, 1, 0, *_rule(), None, None, 0, 0, None, None, None, None, None, None, None, None) == kmc.ERR_ARG


def test_thresholds_at_the_edge(kmc, oracle):
    """min_strong, min_permille and min_len each at the value that just passes a read and the one that just fails it"""
    k = 31
    sample, reads = ti.genome_reads(k, 21, n_reads=60, genome=900)
    kc, table = _counter(kmc, oracle, sample, k, True)
    words = [tm.read_words(r, k, True, gm.solid_set(table, 2, 0)) for r in reads]
    r = next(i for i, w in enumerate(words) if 0 < w[1] < w[0] and w[1] * 1000 % w[0])     # some strong, some weak, no whole permille
    V, S = words[r][:2]
    n_long = words[r][5] + k - 1
    rules = [dict(mode=tm.NONE, min_strong=S), dict(mode=tm.NONE, min_strong=S + 1), dict(mode=tm.NONE, min_permille=S * 1000 // V),
             dict(mode=tm.NONE, min_permille=S * 1000 // V + 1), dict(mode=tm.LONGEST, min_len=n_long), dict(mode=tm.LONGEST, min_len=n_long + 1),
             dict(mode=tm.NONE, min_len=len(reads[r])), dict(mode=tm.NONE, min_len=len(reads[r]) + 1), dict(mode=tm.NONE, min_permille=1000),
             dict(mode=tm.ENDS, min_strong=S, min_permille=S * 1000 // V, min_len=k)]
    with kc:
        seen = _check(kmc, kc, table, True, reads, ((2, 0),), rules)
    own = [bool(seen[((2, 0), i)].verdict[r] & tm.PASS) for i in range(len(rules))]
    assert own == [True, False, True, False, True, False, True, False, False, True]


def test_edge_states(kmc, oracle):
    k = 31
    sample, reads = ti.genome_reads(k, 5, n_reads=40, genome=600)
    bases, offs = ti.pack(reads)
    with kmc.KmerCounter(k=k) as kc:
        # an empty view makes nothing strong
        kc.finalize()
        for kw in MODES:
            m = tm.trim_reads({}, True, reads, 1, 0, k=k, **kw)
            r = kc.trim_reads(bases, offs, 1, 0, *_rule(**kw))
            _equal((r.bases, r.offsets, r.origin, r.stats, r.verdict), _want(m), ("empty view", kw))
            assert r.summary.words() == m.summary and m.summary[2] == 0 and m.summary[1] > 0
        assert len(kc.trim_reads(bases, offs, 1, 0, tm.LONGEST)) == 0 and len(kc.trim_reads(bases, offs, 1, 0, tm.NONE)) == len(reads)
    kc, table = _counter(kmc, oracle, sample, k, True)
    with kc:
        # n_reads == 0
        L = kmc.lib()
        r = kc.trim_reads(np.zeros(0, U8), np.zeros(1, U64))
        assert r.summary.words() == [0] * 8 and len(r.bases) == 0 and list(r.offsets) == [0] and len(r.origin) == 0 and len(r) == 0
        n1, n2 = C.c_uint64(9), C.c_uint64(9)
        w = (C.c_uint64 * 8)(*([7] * 8))
        oo = np.full(2, 0xEEEE, U64)
        assert L.kmc_trim(kc._h, 1, 0, *_rule(), None, None, 0, None, 0, oo.ctypes.data, None, 0, None, None, C.byref(n1), C.byref(n2), w) == 0
        assert (n1.value, n2.value, list(w), oo.tolist()) == (0, 0, [0] * 8, [0, 0xEEEE])
        *p, no, nb, s = kc.trim_reads_device(0, 0, 0, 0)
        assert (no, nb, s.words()) == (0, 0, [0] * 8) and _dev_u64(p[1], 1).tolist() == [0]


@pytest.mark.parametrize("canonical", [True, False])
def test_pipeline_on_the_device(kmc, oracle, canonical):
    """count, trim a noisy batch with LONGEST at range (2, 0), count the device result in a second ctx: every key of that table
    is solid in the first; trimming the result again returns it unchanged"""
    k = 31
    sample, reads = ti.genome_reads(k, 300 + k)
    kc, table = _counter(kmc, oracle, sample, k, canonical)
    m = tm.trim_reads(table, canonical, reads, 2, 0, mode=tm.LONGEST)
    ob, oo = ti.pack(m.out)
    want = oracle.count_kmers(ob, oo, k, canonical)
    bases, offs = ti.pack(reads)
    with kc, kmc.KmerCounter(k=k, canonical=canonical) as second:
        db, do = _upload(bases, offs)
        *p, no, nb, s = kc.trim_reads_device(db.data_ptr(), do.data_ptr(), len(reads), len(bases), 2, 0, tm.LONGEST)
        assert s.words() == m.summary and (no, nb) == (len(m.out), len(ob)) and s.cut_reads >= 30
        second.add_batch_device(p[0], p[1], no, nb, 0)
        t = second.export()
        assert t.equals(want) and t.n_distinct > 1000
        counts = kc.query(t.key_lo, t.key_hi)
        assert len(counts) == t.n_distinct and int(np.min(counts)) >= 2
        # the last call's own arrays handed back in
        *p2, no2, nb2, s2 = kc.trim_reads_device(p[0], p[1], no, nb, 2, 0, tm.LONGEST)
        got = _read_back(p2, no2, nb2, no)
        assert (no2, nb2) == (no, nb) and s2.valid_windows == s2.strong_windows == sum(len(x) - k + 1 for x in m.out) and s2.cut_reads == 0
        assert np.array_equal(got[0], ob) and np.array_equal(got[1], oo) and np.array_equal(got[2], np.arange(no, dtype=U64))


def test_trim_leaves_the_other_results_alone(kmc, oracle):
    """the arrays a correct call, a map call and a unitigs call handed out are byte-identical before and after a trim call"""
    k = 31
    sample, reads = ti.genome_reads(k, 77)
    kc, table = _counter(kmc, oracle, sample, k, True)
    bases, offs = ti.pack(reads)
    nr, nb = len(reads), len(bases)
    with kc:
        db, do = _upload(bases, offs)
        du = kc.unitigs_device(1, 0)
        u_ptrs, (nu, ub) = du[:4], du[4:6]
        mp = kc.map_reads_device(db.data_ptr(), do.data_ptr(), nr, nb, 1, 0)
        dc, ds, dco, dr, nc, _ = kc.correct_reads_device(db.data_ptr(), do.data_ptr(), nr, nb, 2, 0)
        assert nc > 10
        snap = lambda: [_dev_bytes(dc, nb), _dev_bytes(ds, 16 * nr), _dev_bytes(dco, 8 * (nr + 1)), _dev_bytes(dr, 16 * nc),
                        _dev_bytes(mp[0], 8 * nb), _dev_bytes(mp[1], 16 * nr), _dev_bytes(mp[2], 8 * (nr + 1)),
                        _dev_bytes(u_ptrs[0], ub), _dev_bytes(u_ptrs[1], 8 * (nu + 1)), _dev_bytes(u_ptrs[2], 8 * nu)]
        before = snap()
        for kw in MODES:
            kc.trim_reads_device(db.data_ptr(), do.data_ptr(), nr, nb, 2, 0, *_rule(**kw))
            kc.trim_reads(bases, offs, 1, 0, *_rule(**kw))
        after = snap()
        assert all(np.array_equal(a, b) for a, b in zip(before, after))


@pytest.mark.parametrize("forward", [False, True])
def test_cli_trim(kmc, forward):
    k, canonical = 31, not forward
    reads = _sample_reads(kmc)
    table = gm.count_table(reads, k, canonical)
    fw = ["--forward"] if forward else []
    run = lambda *a: subprocess.run([EXE, SAMPLE, "-k", str(k), "--trim", SAMPLE] + list(a) + fw, capture_output=True, text=True)
    r = run()
    assert r.returncode == 0 and r.stdout == tm.trim_reads(table, canonical, reads).text(), r.stderr
    r = run("--min-count", "2")
    assert r.returncode == 0 and r.stdout == tm.trim_reads(table, canonical, reads, 2, 0).text(), r.stderr
    r = run("--min-count", "2", "--trim-mode", "ends", "--min-strong", "5", "--strong-permille", "500", "--min-len", "40")
    assert r.returncode == 0 and r.stdout == tm.trim_reads(table, canonical, reads, 2, 0, mode=tm.ENDS, min_strong=5, min_permille=500, min_len=40).text()
    r = run("--min-count", "2", "--trim-mode", "none", "--invert", "--strong-permille", "900")
    assert r.returncode == 0 and r.stdout == tm.trim_reads(table, canonical, reads, 2, 0, mode=tm.NONE, flags=tm.INVERT, min_permille=900).text()
    if len(reads) % 2 == 0:
        r = run("--min-count", "2", "--paired", "both", "--strong-permille", "900")
        assert r.returncode == 0 and r.stdout == tm.trim_reads(table, canonical, reads, 2, 0, flags=tm.PAIR_BOTH, min_permille=900).text()
    if not forward:
        final = bm.rounds(table, canonical, max_bubble=31, n_rounds=1)[0]
        r = run("--clean", "1", "--bubble-keys", "31")
        assert r.returncode == 0 and r.stdout == tm.trim_reads(final, canonical, reads, k=k).text(), r.stderr
    for bad in (["--map", SAMPLE], ["--profile", SAMPLE], ["--correct", SAMPLE], ["--graph"], ["--histo", "5"], ["--invert"]):
        assert run(*bad).returncode == 2
    assert subprocess.run([EXE, SAMPLE, "--trim", SAMPLE], capture_output=True).returncode == 2      # needs -k
