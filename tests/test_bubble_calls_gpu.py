"""GPU checks of kmc_unitig_bubbles / kmc_unitig_bubbles_device, KmerCounter.bubbles / bubbles_device and `k-mer-count
--variants` (kmc_bubbles.hip.h).  Expected values come from tests/bubble_call_model.py -- the bubbles block of include/kmc.h
on the unitigs and links of unitig_model.py / links_model.py -- applied to the CPU oracle's table of the same input.  All
comparisons are exact: every word of every record and the eight summary words, through every form of the call."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import bubble_call_model as bcm
import bubble_inputs as bi
import bubble_model as bm
import graph_model as gm
from clean_inputs import rnd
from conftest import ROOT, SAMPLE
from test_bubble_calls_host import EVERYTHING_SEED, run_deletion
from test_clean_gpu import _counter, _merged
from test_links_gpu import _dev_u32
from test_unitig_gpu import _dev_bytes, _dev_u64

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "bin", "k-mer-count")
U32, U64 = np.uint32, np.uint64
MODES = (True, False)


def _raw(kmc, kc, lo, hi, lim, nr, nu, spare=3):
    """kmc_unitig_bubbles through ctypes into an array with `spare` records more than needed, filled with a pattern"""
    L = kmc.lib()
    rec = np.full((nr + spare, 8), 0xEEEEEEEE, U32)
    n1, n2 = C.c_uint64(12345), C.c_uint64(12345)
    w = (C.c_uint64 * (kmc.BUBBLE_WORDS + 2))(*([0xEEEE] * 10))
    kc._chk(L.kmc_unitig_bubbles(kc._h, lo, hi, lim, rec.ctypes.data, nr + spare, C.byref(n1), C.byref(n2), w))
    assert (n1.value, n2.value) == (nr, nu) and list(w)[8:] == [0xEEEE] * 2
    assert (rec[nr:] == 0xEEEEEEEE).all()
    return rec[:nr], list(w)[:8]


def _check(kmc, kc, table, canonical, lim, lo=1, hi=0):
    """every form of the call against the model; returns the model's result"""
    L = kmc.lib()
    c = bcm.calls(table, canonical, lo, hi, lim)
    want = np.array(c.records, U32).reshape(len(c.records), 8)
    words, nr, nu = c.summary, c.summary[1], c.summary[0]
    ctx = (kc.k, canonical, lo, hi, lim)
    # the sizing call
    n1, n2 = C.c_uint64(1), C.c_uint64(1)
    w = (C.c_uint64 * 8)()
    kc._chk(L.kmc_unitig_bubbles(kc._h, lo, hi, lim, None, 0, C.byref(n1), C.byref(n2), w))
    assert (n1.value, n2.value, list(w)) == (nr, nu, words), (ctx, list(w), words)
    got, w = _raw(kmc, kc, lo, hi, lim, nr, nu)
    assert w == words, (ctx, w, words)
    assert np.array_equal(got, want), (ctx, got.tolist(), c.records)
    # the device form, read back
    d, dnr, dnu, s = kc.bubbles_device(lo, hi, lim)
    assert (dnr, dnu, s.words()) == (nr, nu, words) and d and d % 8 == 0, (ctx, s.words(), words)
    assert np.array_equal(_dev_u32(d, 8 * nr).reshape(nr, 8), want), ctx
    b = kc.bubbles(lo, hi, lim)
    assert np.array_equal(b.records, want) and b.summary.words() == words and b.records.dtype == U32
    assert b.arms() == c.arms and b.alleles() == c.alleles() and b.to_text() == c.text()
    assert [r[0] for r in c.records] == sorted(r[0] for r in c.records)
    # what simplify pops with tip and island limits 0
    s = kc.simplify_unitigs(lo, hi, 0, 0, lim).summary.words()
    assert s[8:11] == [words[1], words[7], words[2]], (ctx, s, words)
    return c


@pytest.mark.parametrize("canonical", MODES)
@pytest.mark.parametrize("k", [31, 32, 63])
def test_everything(kmc, oracle, k, canonical):
    """every small builder in one table, limit k + 1: nine records, all three kinds, in a canonical ctx reversed arms"""
    kc, table = _counter(kmc, oracle, bi.everything(k, EVERYTHING_SEED[k]), k, canonical)
    with kc:
        c = _check(kmc, kc, table, canonical, k + 1)
        assert c.summary[1] == 9 and c.summary[3] and c.summary[4] and c.summary[5] and bool(c.summary[6]) == canonical
        assert _check(kmc, kc, table, canonical, k).summary[1] == 8            # the arm of k + 1 keys is no candidate any more
        _check(kmc, kc, table, canonical, k + 1, 2, 0)                         # another range: the error arms are not solid


@pytest.mark.parametrize("canonical", MODES)
def test_substitution_k5(kmc, oracle, canonical):
    kc, table = _counter(kmc, oracle, bi.substitution(5, 15)[0], 5, canonical)
    with kc:
        c = _check(kmc, kc, table, canonical, 5)
        assert c.summary[1:6] == [1, 2, 1, 0, 0] and c.records[0][4:6] == [4, 4]


@pytest.mark.parametrize("canonical", MODES)
@pytest.mark.parametrize("k", [31, 32])
def test_deletion_in_a_run(kmc, oracle, k, canonical):
    kc, table = _counter(kmc, oracle, run_deletion(k, 700 + k)[0], k, canonical)
    with kc:
        c = _check(kmc, kc, table, canonical, k)
        assert c.summary[1:6] == [1, 2, 0, 1, 0] and c.records[0][4:6] == [k - 1, k - 3]


@pytest.mark.parametrize("canonical", MODES)
def test_field_of_bubbles(kmc, oracle, canonical):
    """320 records of 1280 unitigs: five workgroups of the pair pass, 80 of the difference pass, records in ascending u"""
    k = 31
    kc, table = _counter(kmc, oracle, bi.field(k, 100 + k)[0], k, canonical)
    with kc:
        c = _check(kmc, kc, table, canonical, k)
        assert c.summary[:6] == [1280, 320, 640, 320, 0, 0] and all(r[4:6] == [30, 30] for r in c.records)


def _spaced(k, offsets, seed):
    """a sequence read three times and one read that changes the positions 3k + o for o in offsets: where every window
    between the first and the last of them holds a changed base, one arm of k + offsets[-1] keys"""
    rng = np.random.default_rng(seed)
    s = rnd(rng, 6 * k + offsets[-1])
    e = list(s)
    for o in offsets:
        e[3 * k + o] = bi._other(rng, s[3 * k + o])
    return [s] * 3 + ["".join(e)[3 * k - (k - 1):3 * k + offsets[-1] + k]]


@pytest.mark.parametrize("canonical", MODES)
@pytest.mark.parametrize("k,offsets,arm,mism", [(31, (0, 20, 40), 101, 3), (63, (0, 40), 165, 2)])
def test_arms_of_several_steps(kmc, oracle, k, offsets, arm, mism, canonical):
    """an arm of 101 bases at k = 31 (two steps of 64 positions) and one of 165 at k = 63 (three), limit k + 40"""
    kc, table = _counter(kmc, oracle, _spaced(k, offsets, 300 + k), k, canonical)
    with kc:
        c = _check(kmc, kc, table, canonical, k + 40)
        assert c.summary[1:6] == [1, 2, 0, 0, 1] and c.records[0][4:] == [k - 1, k - 1, bcm.COMPLEX | (c.records[0][6] & 4), mism]
        assert [len(a) for a in c.arms[0]] == [arm, arm] and [len(a) for a in c.alleles()[0]] == [41, 41]
        assert _check(kmc, kc, table, canonical, k + 39).summary[1:3] == [0, 0]


@pytest.mark.parametrize("canonical", MODES)
def test_two_substitutions_40_apart_at_k31(kmc, oracle, canonical):
    """farther apart than k - 1 the two substitutions are two bubbles of k keys with nine true keys between them"""
    k = 31
    kc, table = _counter(kmc, oracle, _spaced(k, (0, 40), 331), k, canonical)
    with kc:
        c = _check(kmc, kc, table, canonical, k + 40)
        assert c.summary[1:6] == [2, 4, 2, 0, 0]


@pytest.mark.parametrize("canonical", MODES)
@pytest.mark.parametrize("k", [31, 63])
def test_wide_products_pick_the_major(kmc, k, canonical):
    """mean abundances whose comparison needs more than 64 bits of product: the arm of k keys is the major one"""
    table, true_arm, ins_arm = bi.wide_bubble(k, canonical, 50 + k)
    with _merged(kmc, table, k, canonical) as kc:
        c = _check(kmc, kc, table, canonical, k)
    assert c.summary[1:6] == [1, 2, 0, 1, 0]
    assert c.records[0][:2] == [bi.unitig_with(c.unitigs, true_arm[0], k, canonical), bi.unitig_with(c.unitigs, ins_arm[0], k, canonical)]
    assert c.summary[7] == k - 1 and [len(a) for a in c.alleles()[0]] == [0, 1]


_CHILD = r"""
import importlib, sys
sys.path.insert(0, sys.argv[1])
kmc = importlib.import_module("k-mer-count_amd")
bases, offs = kmc.parse_fasta(sys.argv[2])
with kmc.KmerCounter(k=31) as kc:
    kc.add_batch(bases, offs)
    kc.finalize()
    step = lambda s: print("step " + s, file=sys.stderr, flush=True)
    step("links(1,0)")
    kc.unitig_links(1, 0)
    step("bubbles(1,0)")
    a = kc.bubbles(1, 0)
    step("bubbles(1,0) again")
    b = kc.bubbles(1, 0)
    assert (a.records == b.records).all()
    step("simplify(1,0) between")
    kc.simplify_unitigs(1, 0)
    kc.bubbles(1, 0)
    kc.simplify_unitigs(1, 0)
    step("bubbles(1,0) other limit")
    kc.bubbles(1, 0, 93)
    step("bubbles_device(1,0)")
    kc.bubbles_device(1, 0, 93)
    step("graph(2,0) bubbles(1,0)")
    kc.graph(2, 0, adj=False)
    kc.bubbles_device(1, 0)
    step("bubbles(2,0)")
    kc.bubbles(2, 0)
    step("end")
"""


def test_bubbles_reuse_the_held_unitigs_and_links(kmc):
    """What computes, seen through the KMC_UNITIG_TRACE lines of a child process (nothing is timed)"""
    env = dict(os.environ, KMC_UNITIG_TRACE="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, SAMPLE], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    steps, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("step "):
            cur = line[5:]
            steps[cur] = []
        elif line.split(":")[0] in ("kmc_unitigs", "kmc_unitig_links", "kmc_unitig_clean", "kmc_unitig_simplify", "kmc_unitig_bubbles"):
            steps[cur].append(line.split(":")[0])
            if line.startswith("kmc_unitig_bubbles:"):
                assert line.split()[1::2] == ["keys", "unitigs", "candidates", "records", "subst", "indel", "complex", "reversed", "pair_ms", "diff_ms"], line
    assert steps["links(1,0)"] == ["kmc_unitigs", "kmc_unitig_links"]
    # behind the links of the same range: neither a unitigs nor a links line, and sizing, the unitigs' copy and the copy are one pass
    assert steps["bubbles(1,0)"] == ["kmc_unitig_bubbles"]
    assert steps["bubbles(1,0) again"] == []
    # a simplify result and a bubbles result do not end one another
    assert steps["simplify(1,0) between"] == ["kmc_unitig_simplify"]
    # the limit is part of the key of the held result
    assert steps["bubbles(1,0) other limit"] == ["kmc_unitig_bubbles"]
    # the device form always runs the pass
    assert steps["bubbles_device(1,0)"] == ["kmc_unitig_bubbles"]
    # a graph call has rewritten adj: both are computed again
    assert steps["graph(2,0) bubbles(1,0)"] == ["kmc_unitigs", "kmc_unitig_links", "kmc_unitig_bubbles"]
    assert steps["bubbles(2,0)"] == ["kmc_unitigs", "kmc_unitig_links", "kmc_unitig_bubbles"]


def test_nothing_else_moved(kmc, oracle):
    """the arrays a preceding unitigs, links or simplify call handed out are unchanged by the bubbles calls behind them"""
    k = 31
    kc, table = _counter(kmc, oracle, bi.everything(k, EVERYTHING_SEED[k]) + bi.field(k, 100 + k, 40)[0], k, True)
    with kc:
        kc.finalize()
        digest = kc.export().digest()
        db, do, da, df, nu, nb, _ = kc.unitigs_device(1, 0)
        lo_, lt, lnu, nl, _ = kc.unitig_links_device(1, 0)
        shi, slo, scnt, sv, nk, snu, sw = kc.simplify_unitigs_device(1, 0)
        assert nu == lnu == snu and sw.bubbles > 40
        read = lambda: [_dev_u64(p, m) for p, m in ((slo, nk), (scnt, nk), (do, nu + 1), (da, nu), (lo_, 2 * nu + 1))] + \
                       [_dev_bytes(sv, nu), _dev_bytes(db, nb), _dev_bytes(df, nu), _dev_u32(lt, nl)]
        before = read()
        c = bcm.calls(table, True, 1, 0, k)
        want = np.array(c.records, U32).reshape(-1, 8)
        d, nr, dnu, s = kc.bubbles_device(1, 0)
        assert (nr, dnu, s.words()) == (len(want), nu, c.summary) and np.array_equal(_dev_u32(d, 8 * nr).reshape(nr, 8), want)
        b = kc.bubbles(1, 0, k + 1)
        assert b.summary.records == nr + 1
        after = read()
        assert all(np.array_equal(x, y) for x, y in zip(before, after))
        assert np.array_equal(after[5], np.array(bm.simplify(table, True).verdict, np.uint8))
        # and the simplify result is still the one the ctx holds: the host form copies it
        again = kc.simplify_unitigs(1, 0)
        assert np.array_equal(again.verdict, after[5]) and np.array_equal(again.table.key_lo, after[0])
        assert kc.export().digest() == digest


def test_state_errors_and_limits(kmc, oracle):
    L = kmc.lib()
    k = 31
    reads = bi.substitution(k, 10 + k)[0]
    n1, n2 = C.c_uint64(99), C.c_uint64(99)
    w = (C.c_uint64 * 8)(*([7] * 8))
    p = C.c_void_p(1)

    def host(kc, lo, hi, lim=k):
        return L.kmc_unitig_bubbles(kc._h, lo, hi, lim, None, 0, C.byref(n1), C.byref(n2), w)

    def device(kc, lo, hi, lim=k):
        return L.kmc_unitig_bubbles_device(kc._h, lo, hi, lim, C.byref(p), C.byref(n1), C.byref(n2), w)

    with kmc.KmerCounter(k=k) as kc:
        assert host(kc, 1, 0) == kmc.ERR_STATE and device(kc, 1, 0) == kmc.ERR_STATE          # no view: before any finalize
    kc, table = _counter(kmc, oracle, reads, k, True)
    with kc:
        kc.finalize()
        # every output pointer may be NULL
        assert L.kmc_unitig_bubbles_device(kc._h, 1, 0, k, None, None, None, None) == kmc.OK
        assert L.kmc_unitig_bubbles(kc._h, 1, 0, k, None, 0, None, None, None) == kmc.OK
        # max below min
        assert host(kc, 3, 2) == kmc.ERR_ARG and device(kc, 3, 2) == kmc.ERR_ARG
        c = bcm.calls(table, True)
        assert host(kc, 1, 0) == kmc.OK and (n1.value, n2.value, list(w)) == (1, 4, c.summary)
        # limit 0: no records, no candidates; 2^31 or more: an argument error in both forms, the held result untouched
        assert host(kc, 1, 0, 0) == kmc.OK and (n1.value, n2.value, list(w)) == (0, 4, [4, 0, 0, 0, 0, 0, 0, 0])
        assert device(kc, 1, 0, 0) == kmc.OK and (n1.value, n2.value, list(w)) == (0, 4, [4, 0, 0, 0, 0, 0, 0, 0]) and p.value
        for lim in (1 << 31, (1 << 31) + 5, (1 << 64) - 1):
            assert host(kc, 1, 0, lim) == kmc.ERR_ARG and b"kmc_unitig_bubbles" in L.kmc_last_error(kc._h)
            assert device(kc, 1, 0, lim) == kmc.ERR_ARG
        with pytest.raises(kmc.KmcError) as e:
            kc.bubbles(max_bubble_keys=1 << 31)
        assert e.value.status == kmc.ERR_ARG
        assert host(kc, 1, 0, (1 << 31) - 1) == kmc.OK and (n1.value, list(w)) == (1, c.summary)
        # nothing solid
        assert host(kc, 10 ** 9, 0) == kmc.OK and (n1.value, n2.value, list(w)) == (0, 0, [0] * 8)
        assert device(kc, 10 ** 9, 0) == kmc.OK and (n1.value, n2.value, list(w)) == (0, 0, [0] * 8)
        # a cap one too small: the sizes are set, nothing is copied
        rec = np.full((1, 8), 0xEEEEEEEE, U32)
        n1.value = n2.value = 0
        assert L.kmc_unitig_bubbles(kc._h, 1, 0, k, rec.ctypes.data, 0, C.byref(n1), C.byref(n2), w) == kmc.ERR_ARG
        assert (n1.value, n2.value) == (1, 4) and (rec == 0xEEEEEEEE).all() and b"kmc_unitig_bubbles" in L.kmc_last_error(kc._h)
        assert L.kmc_unitig_bubbles(kc._h, 1, 0, k, rec.ctypes.data, 1, None, None, None) == kmc.OK and rec.tolist() == c.records
        # an empty view
        kc.reset()
        assert host(kc, 1, 0) == kmc.ERR_STATE and device(kc, 1, 0) == kmc.ERR_STATE
        kc.finalize()
        b = kc.bubbles()
        assert b.records.shape == (0, 8) and b.summary.words() == [0] * 8 and b.to_text() == ""
        assert kc.bubbles_device()[1:3] == (0, 0)
    with kmc.KmerCounter(mode=kmc.MODE_LR) as kc:
        kc.count_file(SAMPLE)
        kc.finalize()
        assert host(kc, 1, 0) == kmc.ERR_ARG and device(kc, 1, 0) == kmc.ERR_ARG
        with pytest.raises(kmc.KmcError) as e:
            kc.bubbles()
        assert e.value.status == kmc.ERR_ARG


@pytest.mark.parametrize("forward", [False, True])
def test_cli_variants(kmc, tmp_path, forward):
    k = 31
    canonical = not forward
    reads = bi.everything(k, EVERYTHING_SEED[k])
    fa = tmp_path / "variants.fasta"
    fa.write_text("".join(">r%d\n%s\n" % (i, s) for i, s in enumerate(reads)))
    table = gm.count_table(reads, k, canonical)
    fw = ["--forward"] if forward else []
    run = lambda *a: subprocess.run([EXE, str(fa), "-k", str(k), "--variants"] + list(a) + fw, capture_output=True, text=True)
    c = bcm.calls(table, canonical, max_bubble=k + 1)
    r = run("--bubble-keys", str(k + 1))
    assert r.returncode == 0 and r.stdout == c.text() and len(r.stdout.splitlines()) == 9, r.stderr
    assert {l.split("\t")[1] for l in r.stdout.splitlines()} == {"S", "I", "C"} and any("\t-\t" in l for l in r.stdout.splitlines())
    r = run()                                                                   # the default limit is k
    assert r.returncode == 0 and r.stdout == bcm.calls(table, canonical).text() and len(r.stdout.splitlines()) == 8, r.stderr
    r = run("--min-count", "2")
    assert r.returncode == 0 and r.stdout == bcm.calls(table, canonical, 2, 0).text(), r.stderr
    r = run("--bubble-keys", "0")
    assert r.returncode == 0 and r.stdout == "", r.stderr
    # behind a cleaning round (which with --variants pops no bubble): the variants of the cleaned table
    cleaned = bm.cm.rounds(table, canonical, n_rounds=1)[0]
    r = run("--clean", "1", "--bubble-keys", str(k + 1))
    assert r.returncode == 0 and r.stdout == bcm.calls(cleaned, canonical, max_bubble=k + 1).text() and r.stdout, r.stderr
