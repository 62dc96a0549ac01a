"""GPU checks of kmc_normalize / kmc_normalize_device / KmerCounter.normalize_reads (kmc_normalize.hip.h).  Expected values
come from tests/normalize_model.py -- the definitions of include/kmc.h on Python strings -- applied to the table the ctx was
loaded with.  All comparisons are exact, entry by entry, through every form of the call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bubble_model as bm
import graph_model as gm
import normalize_inputs as ni
import normalize_model as nm
import trim_inputs as ti
import trim_model as tm
from conftest import ROOT, SAMPLE
from test_correct_gpu import _counter, _sample_reads, _upload
from test_unitig_gpu import _dev_bytes, _dev_u64

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "bin", "k-mer-count")
U64, U32, U8 = np.uint64, np.uint32, np.uint8
NAMES = ("bases", "offsets", "origin", "stats", "verdict")
# the select kernel's variants, in windows (kmc_normalize.hip.h: "#define KMC_NM_SLOTS 16", KMC_NM_WAVE_MAX = 64 * KMC_NM_SLOTS)
WAVE_MAX = 1024


def _rule(permille=500, target=0, min_depth=0, seed=0, flags=0):
    return permille, target, min_depth, seed, flags


def _loaded(kmc, table, k, canonical):
    """a ctx whose view is `table`, loaded as (key, count) pairs"""
    import torch
    hi, lo, cnt = ni.pairs_arrays(kmc, table)
    kc = kmc.KmerCounter(k=k, canonical=canonical)
    if len(lo):
        d = [torch.from_numpy(a.view(np.int64)).cuda() for a in (hi, lo, cnt)]
        torch.cuda.synchronize()
        kc.merge_pairs_device(d[0].data_ptr() if k > 32 else 0, d[1].data_ptr(), d[2].data_ptr(), len(lo))
    nd, nt = kc.finalize()
    assert (nd, nt) == (len(table), sum(table.values()))
    return kc


def _want(m):
    return (np.frombuffer("".join(m.out).encode(), U8), np.array(m.offsets, U64), np.array(m.origin, U64),
            np.array(m.stats, U32).reshape(-1, 4), np.array(m.verdict, U8))


def _equal(got, want, ctx):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.size == w.size, (ctx, name, g.dtype, g.shape, w.shape)
        g = g.reshape(w.shape)
        bad = np.flatnonzero((g != w).reshape(len(w), -1).any(axis=1))[:5] if w.size else []
        assert not len(bad), (ctx, name, bad, g[bad], w[bad])


def _host(kmc, kc, rule, bases, offs, *arrays):
    """kmc_normalize through ctypes; arrays: out_bases, cap_bases, out_offsets, origin, cap_reads, read_stats, verdict"""
    n1, n2 = C.c_uint64(12345), C.c_uint64(12345)
    w = (C.c_uint64 * kmc.NORMALIZE_WORDS)()
    nr = len(offs) - 1
    rc = kmc.lib().kmc_normalize(kc._h, *rule, bases.ctypes.data if nr else None, offs.ctypes.data if nr else None, nr, *arrays,
                                 C.byref(n1), C.byref(n2), w)
    return rc, n1.value, n2.value, list(w)


def _raw(kmc, kc, rule, bases, offs, no, nb, spare=3):
    """the host form into arrays with `spare` entries more than needed, filled with a pattern"""
    nr = len(offs) - 1
    out, oo, org = np.full(nb + spare, 0xEE, U8), np.full(no + 1 + spare, 0xEEEE, U64), np.full(no + spare, 0xEEEE, U64)
    stats, verdict = np.full(4 * nr + spare, 0xEEEEEEEE, U32), np.full(nr + spare, 0xEE, U8)
    rc, n1, n2, w = _host(kmc, kc, rule, bases, offs, out.ctypes.data, nb + spare, oo.ctypes.data, org.ctypes.data, no + spare, stats.ctypes.data,
                          verdict.ctypes.data)
    assert (rc, n1, n2) == (0, no, nb)
    assert (out[nb:] == 0xEE).all() and (oo[no + 1:] == 0xEEEE).all() and (org[no:] == 0xEEEE).all()
    assert (stats[4 * nr:] == 0xEEEEEEEE).all() and (verdict[nr:] == 0xEE).all()
    return (out[:nb], oo[:no + 1], org[:no], stats[:4 * nr], verdict[:nr]), w


def _read_back(p, no, nb, nr):
    db, doo, dorg, ds, dv = p
    assert db % 16 == 0 and doo % 8 == 0 and dorg % 8 == 0 and ds % 16 == 0
    padded = _dev_bytes(db, (nb + 15) // 16 * 16)
    assert not padded[nb:].any()                     # zero up to the 16-byte boundary
    return padded[:nb], _dev_u64(doo, no + 1), _dev_u64(dorg, no), _dev_bytes(ds, 16 * nr).view(U32), _dev_bytes(dv, nr)


def _check(kmc, kc, table, canonical, reads, rules, counts=None):
    """every form of the call against the model, for every rule; returns the model's results"""
    bases, offs = ni.pack(reads)
    nr = len(reads)
    counts = counts if counts is not None else nm.all_counts(table, canonical, reads, kc.k)
    db, do = _upload(bases, offs)
    seen = []
    for kw in rules:
        m = nm.normalize_reads(table, canonical, reads, kc.k, counts, **kw)
        rule = _rule(**kw)
        want, summary = _want(m), m.summary
        no, nb = summary[2], summary[3]
        ctx = (kc.k, canonical, rule)
        # the sizing call
        rc, n1, n2, w = _host(kmc, kc, rule, bases, offs, None, 0, None, None, 0, None, None)
        assert (rc, n1, n2, w) == (0, no, nb, summary), (ctx, rc, n1, n2, w, summary)
        got, w = _raw(kmc, kc, rule, bases, offs, no, nb)
        assert w == summary, (ctx, w, summary)
        _equal(got, want, ctx + ("host",))
        *p, dno, dnb, s = kc.normalize_reads_device(db.data_ptr(), do.data_ptr(), nr, len(bases), kw.get("target", 0), kw.get("permille", 500),
                                                    kw.get("min_depth", 0), kw.get("seed", 0), kw.get("flags", 0))
        assert (dno, dnb, s.words()) == (no, nb, summary), (ctx, dno, dnb, s.words(), summary)
        _equal(_read_back(p, dno, dnb, nr), want, ctx + ("device",))
        r = kc.normalize_reads(bases, offs, kw.get("target", 0), kw.get("permille", 500), kw.get("min_depth", 0), kw.get("seed", 0), kw.get("flags", 0))
        _equal((r.bases, r.offsets, r.origin, r.stats, r.verdict), want, ctx + ("normalize_reads",))
        assert r.summary.words() == summary and len(r) == no and r.strings() == m.out and r.to_fasta() == m.text()
        seen.append(m)
    return seen


def _mid_depth(counts):
    d = sorted(nm.depth(c, 500)[1] for c in counts)
    return d[len(d) // 2]


CASES = [(5, "spread"), (33, "spread")] + [(31, v) for v in ni.VARIANTS]


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k,variant", CASES)
def test_lengths_permilles_and_counts(kmc, k, variant, canonical):
    """reads below k, of 1, 2, 63, 64, 65 windows, on both sides of the wave / workgroup boundary and a workgroup read off 256;
    an all-N read, N and lower case inside, a read of absent windows, empty reads among the emitted; every permille; counts
    that decide in every digit pass, in the top byte alone, in the low byte alone, with many ties, and above 32 bits"""
    assert ni.WAVE_MAX == WAVE_MAX
    table, reads, names = ni.table_and_reads(k, 3 + k, canonical, variant)
    counts = nm.all_counts(table, canonical, reads, k)
    T = _mid_depth(counts)
    rules = [dict(permille=p, target=T, seed=p) for p in ni.PERMILLES]
    rules += [dict(permille=500, target=T, min_depth=1, seed=3), dict(permille=500, target=T, min_depth=1, seed=3, flags=nm.INVERT),
              dict(permille=1000, target=1 << 33), dict(permille=1000, min_depth=1 << 32), dict()]
    with _loaded(kmc, table, k, canonical) as kc:
        seen = _check(kmc, kc, table, canonical, reads, rules, counts)
        # permille 0 / 1000 against kmc_profile on the same batch
        bases, offs = ni.pack(reads)
        _, ps = kc.profile(bases, offs, windows=False)
    sat = np.minimum(ps, U64(nm.SAT))
    assert [s[0] for s in seen[0].stats] == ps[:, 0].tolist() and [s[1] for s in seen[0].stats] == sat[:, 2].tolist()
    assert [s[1] for s in seen[6].stats] == sat[:, 3].tolist()
    # what the rules were chosen for
    mid = seen[3]
    assert 0 < mid.summary[5] < len(reads) and (variant in ("low", "ties") or 0 < mid.summary[6] < mid.summary[5])
    assert any(not s for s in mid.out)                                                   # empty reads among the emitted
    assert seen[7].summary[4] >= 6 and not any(not s for s in seen[7].out)               # min_depth 1 drops the reads of depth 0
    assert seen[9].stats[names["big"]][1] == nm.SAT and seen[9].summary[5] == 0          # saturated, and not above a target of 2^33
    assert seen[10].summary[4] == len(reads) and seen[10].out == []                      # ... nor at a floor of 2^32
    assert seen[11].out == reads and seen[11].origin == list(range(len(reads)))          # the identity call


def test_paired_and_invert_truth_tables(kmc):
    k = 31
    table, reads = ni.pairs(k, 5)
    rules = [dict(target=40, min_depth=2, seed=1, flags=f) for f in (0, nm.INVERT, nm.PAIRED, nm.PAIRED | nm.INVERT)]
    with _loaded(kmc, table, k, True) as kc:
        seen = _check(kmc, kc, table, True, reads, rules)
    bits = lambda i: [v & 13 for v in seen[i].verdict[:12]]
    em = lambda i: [bool(v & nm.EMITTED) for v in seen[i].verdict]
    D, K, L = nm.DEEP, nm.KEEP, nm.LOW
    assert [b & ~K for b in bits(0)] == [D, 0, 0, D, 0, 0, D, L, L, 0, L, L] and bits(1) == bits(0)
    assert bits(2) == [K, K, K, K, K, K, L, L, L, L, L, L] and bits(3) == bits(2)
    assert em(1) == [not x for x in em(0)] and em(3) == [not x for x in em(2)] and em(2)[:12] == [True] * 6 + [False] * 6
    assert all(em(2)[i] == em(2)[i + 1] for i in range(0, len(reads), 2)) and 0 < sum(em(2)[12:]) < 40


def test_argument_errors_and_edge_states(kmc):
    k = 31
    L = kmc.lib()
    table, reads, names = ni.table_and_reads(k, 34, True)
    bases, offs = ni.pack(reads)
    nr = len(reads)
    sizing = lambda kc, rule, n=nr: L.kmc_normalize(kc._h, *rule, bases.ctypes.data, offs.ctypes.data, n, None, 0, None, None, 0, None, None,
                                                    C.byref(n1), C.byref(n2), None)
    n1, n2 = C.c_uint64(9), C.c_uint64(9)
    with _loaded(kmc, table, k, True) as kc:
        assert nr % 2 == 0 and sizing(kc, _rule(flags=nm.PAIRED)) == 0
        assert sizing(kc, _rule(flags=nm.PAIRED), nr - 1) == kmc.ERR_ARG               # odd n_reads with PAIRED
        assert sizing(kc, _rule(permille=1001)) == kmc.ERR_ARG
        assert sizing(kc, _rule(flags=4)) == kmc.ERR_ARG and sizing(kc, _rule(flags=1 << 31)) == kmc.ERR_ARG     # unknown flag bits
        bad = offs.copy()
        bad[3] = bad[2] - 1
        assert L.kmc_normalize(kc._h, *_rule(), bases.ctypes.data, bad.ctypes.data, nr, None, 0, None, None, 0, None, None, C.byref(n1), C.byref(n2),
                               None) == kmc.ERR_ARG
        assert L.kmc_normalize(kc._h, *_rule(), None, None, nr, None, 0, None, None, 0, None, None, C.byref(n1), C.byref(n2), None) == kmc.ERR_ARG
        assert L.kmc_normalize(None, *_rule(), bases.ctypes.data, offs.ctypes.data, nr, None, 0, None, None, 0, None, None, C.byref(n1), C.byref(n2),
                               None) == kmc.ERR_ARG and (n1.value, n2.value) == (0, 0)
        # target and min_depth above 2^32 are plain comparisons
        assert sizing(kc, _rule(target=1 << 40, min_depth=1 << 35)) == 0 and (n1.value, n2.value) == (0, 0)
        # a cap one too small: KMC_ERR_ARG, the counts are set and nothing is copied; an array that is NULL has no cap
        m = nm.normalize_reads(table, True, reads, k, min_depth=1)
        no, nb = m.summary[2], m.summary[3]
        out, oo, org = np.full(nb, 0xEE, U8), np.full(no + 1, 0xEEEE, U64), np.full(no, 0xEEEE, U64)
        host = lambda *a: _host(kmc, kc, _rule(min_depth=1), bases, offs, *a, None, None)
        assert host(out.ctypes.data, nb - 1, oo.ctypes.data, org.ctypes.data, no)[:3] == (kmc.ERR_ARG, no, nb)
        assert host(out.ctypes.data, nb, oo.ctypes.data, org.ctypes.data, no - 1)[0] == kmc.ERR_ARG
        assert (out == 0xEE).all() and (oo == 0xEEEE).all() and (org == 0xEEEE).all()
        assert host(out.ctypes.data, nb, None, None, 0)[0] == 0 and out.tobytes().decode() == "".join(m.out)
        # the device form: null and misaligned arrays; its own result handed back in
        db, do = _upload(bases, offs)
        dev = lambda b, o, n, nbases: L.kmc_normalize_device(kc._h, *_rule(), b, o, n, nbases, None, None, None, None, None, None, None, None)
        assert dev(None, do.data_ptr(), nr, len(bases)) == kmc.ERR_ARG and dev(db.data_ptr() + 1, do.data_ptr(), nr, len(bases)) == kmc.ERR_ARG
        *p, no, nb, s = kc.normalize_reads_device(db.data_ptr(), do.data_ptr(), nr, len(bases))
        assert (no, nb) == (nr, len(bases))
        assert dev(p[0], p[1], no, nb) == kmc.ERR_ARG and dev(p[0], do.data_ptr(), nr, len(bases)) == kmc.ERR_ARG
        assert dev(db.data_ptr(), p[1], no, nb) == kmc.ERR_ARG
        assert b"own" in L.kmc_last_error(kc._h)
        got = _read_back(p, no, nb, nr)                                                   # the refused calls wrote nothing
        assert np.array_equal(got[0], bases) and np.array_equal(got[1], offs) and np.array_equal(got[2], np.arange(nr, dtype=U64))
        # n_reads == 0
        r = kc.normalize_reads(np.zeros(0, U8), np.zeros(1, U64), target=5)
        assert r.summary.words() == [0] * 8 and len(r.bases) == 0 and list(r.offsets) == [0] and len(r.origin) == 0 and len(r) == 0
        w = (C.c_uint64 * 8)(*([7] * 8))
        oo = np.full(2, 0xEEEE, U64)
        assert L.kmc_normalize(kc._h, *_rule(), None, None, 0, None, 0, oo.ctypes.data, None, 0, None, None, C.byref(n1), C.byref(n2), w) == 0
        assert (n1.value, n2.value, list(w), oo.tolist()) == (0, 0, [0] * 8, [0, 0xEEEE])
        *p, no, nb, s = kc.normalize_reads_device(0, 0, 0, 0, flags=nm.PAIRED)
        assert (no, nb, s.words()) == (0, 0, [0] * 8) and _dev_u64(p[1], 1).tolist() == [0]
    with kmc.KmerCounter(k=k) as fresh:
        assert sizing(fresh, _rule()) == kmc.ERR_STATE                                    # no view
        assert L.kmc_normalize_device(fresh._h, *_rule(), None, None, 0, 0, None, None, None, None, None, None, None, None) == kmc.ERR_STATE
        # an empty view makes every count 0
        fresh.finalize()
        _check(kmc, fresh, {}, True, reads, [dict(), dict(min_depth=1), dict(target=1, permille=1000)])
        assert len(fresh.normalize_reads(bases, offs, min_depth=1)) == 0
    with kmc.KmerCounter(mode=kmc.MODE_LR) as lr:
        assert sizing(lr, _rule()) == kmc.ERR_ARG                                         # LR ctx
        assert L.kmc_normalize_device(lr._h, *_rule(), None, None, 0, 0, None, None, None, None, None, None, None, None) == kmc.ERR_ARG


@pytest.mark.parametrize("canonical", [True, False])
def test_with_trim_and_correct_on_the_device(kmc, oracle, canonical):
    """the normalise result goes into trim_reads_device, a trim result comes in, both against the models; what a trim and a
    correct call handed out is byte-identical after the normalise calls"""
    k = 31
    sample, reads = ti.genome_reads(k, 300 + k)
    kc, table = _counter(kmc, oracle, sample, k, canonical)
    bases, offs = ti.pack(reads)
    nr, nb = len(reads), len(bases)
    counts = nm.all_counts(table, canonical, reads, k)
    T = max(_mid_depth(counts), 1)
    rule = dict(target=T, min_depth=1, seed=4)
    m = nm.normalize_reads(table, canonical, reads, k, counts, **rule)
    assert 0 < m.summary[4] and 0 < m.summary[6] < m.summary[5]
    with kc:
        db, do = _upload(bases, offs)
        dc, ds, dco, dr, nc, _ = kc.correct_reads_device(db.data_ptr(), do.data_ptr(), nr, nb, 2, 0)
        *tp, tno, tnb, ts = kc.trim_reads_device(db.data_ptr(), do.data_ptr(), nr, nb, 2, 0, tm.LONGEST)
        snap = lambda: [_dev_bytes(dc, nb), _dev_bytes(ds, 16 * nr), _dev_bytes(dco, 8 * (nr + 1)), _dev_bytes(dr, 16 * nc), _dev_bytes(tp[0], tnb),
                        _dev_bytes(tp[1], 8 * (tno + 1)), _dev_bytes(tp[2], 8 * tno), _dev_bytes(tp[3], 16 * nr), _dev_bytes(tp[4], nr)]
        before = snap()
        # a trim result comes in
        t = tm.trim_reads(table, canonical, reads, 2, 0, mode=tm.LONGEST)
        assert ts.words() == t.summary and tno > 20
        mt = nm.normalize_reads(table, canonical, t.out, k, **rule)
        *p, no, nob, s = kc.normalize_reads_device(tp[0], tp[1], tno, tnb, **rule)
        assert (no, nob, s.words()) == (mt.summary[2], mt.summary[3], mt.summary)
        _equal(_read_back(p, no, nob, tno), _want(mt), "trim result in")
        # the normalise result goes out, into trim and into a count
        *p, no, nob, s = kc.normalize_reads_device(db.data_ptr(), do.data_ptr(), nr, nb, **rule)
        assert s.words() == m.summary
        kc.normalize_reads(bases, offs, **rule)                                           # (the host form writes the same arrays again: same batch, same rule)
        after = snap()
        assert all(np.array_equal(a, b) for a, b in zip(before, after))
        t2 = tm.trim_reads(table, canonical, m.out, 2, 0, mode=tm.ENDS)
        *q, qno, qnb, qs = kc.trim_reads_device(p[0], p[1], no, nob, 2, 0, tm.ENDS)
        assert qs.words() == t2.summary
        got = (_dev_bytes(q[0], qnb), _dev_u64(q[1], qno + 1), _dev_u64(q[2], qno))
        assert got[0].tobytes().decode() == "".join(t2.out) and got[1].tolist() == t2.offsets and got[2].tolist() == t2.origin
        with kmc.KmerCounter(k=k, canonical=canonical) as second:
            second.add_batch_device(p[0], p[1], no, nob, 0)
            ob, oo = ti.pack(m.out)
            assert second.export().equals(oracle.count_kmers(ob, oo, k, canonical))


@pytest.mark.parametrize("forward", [False, True])
def test_cli_normalize(kmc, forward):
    k, canonical = 31, not forward
    reads = _sample_reads(kmc)
    table = gm.count_table(reads, k, canonical)
    counts = nm.all_counts(table, canonical, reads, k)
    T = max(_mid_depth(counts) // 2, 1)
    fw = ["--forward"] if forward else []
    run = lambda *a: subprocess.run([EXE, SAMPLE, "-k", str(k), "--normalize", SAMPLE] + list(a) + fw, capture_output=True, text=True)
    model = lambda **kw: nm.normalize_reads(table, canonical, reads, k, counts, **kw)
    r = run("--target", str(T))
    assert r.returncode == 0 and r.stdout == model(target=T).text() and 0 < r.stdout.count(">") < len(reads), r.stderr
    r = run("--target", "0")
    assert r.returncode == 0 and r.stdout == model().text() and r.stdout.count(">") == len(reads)
    r = run("--target", str(T), "--depth-permille", "900", "--min-depth", "2", "--seed", "77")
    assert r.returncode == 0 and r.stdout == model(target=T, permille=900, min_depth=2, seed=77).text()
    r = run("--target", str(T), "--norm-invert", "--seed", "77")
    assert r.returncode == 0 and r.stdout == model(target=T, seed=77, flags=nm.INVERT).text()
    if len(reads) % 2 == 0:
        r = run("--target", str(T), "--norm-paired")
        assert r.returncode == 0 and r.stdout == model(target=T, flags=nm.PAIRED).text()
    if not forward:
        final = bm.rounds(table, canonical, max_bubble=31, n_rounds=1)[0]
        r = run("--target", str(T), "--clean", "1", "--bubble-keys", "31")
        assert r.returncode == 0 and r.stdout == nm.normalize_reads(final, canonical, reads, k, target=T).text(), r.stderr
    for bad in (["--map", SAMPLE], ["--profile", SAMPLE], ["--correct", SAMPLE], ["--trim", SAMPLE], ["--graph"], ["--histo", "5"], ["--invert"]):
        assert run("--target", "3", *bad).returncode == 2
    assert run().returncode == 2                                                          # needs --target
    assert subprocess.run([EXE, SAMPLE, "--normalize", SAMPLE, "--target", "3"], capture_output=True).returncode == 2      # needs -k
