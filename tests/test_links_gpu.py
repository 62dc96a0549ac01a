"""GPU checks of kmc_unitig_links / kmc_unitig_links_device / KmerCounter.unitig_links (kmc_links.hip.h).  Expected values
come from tests/links_model.py -- the definition of include/kmc.h applied to the terminal sides that the joins and cycle
cuts of unitig_model.py leave -- on the CPU oracle's table of the same input.  All comparisons are exact: the offsets, the
records in order, and the eight summary words, through every form of the call."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import graph_model as gm
import links_model as lm
import unitig_model as um
from conftest import ROOT, SAMPLE
from test_unitig_gpu import _dev_bytes, _dev_u64, _pack, _rnd, _same, _table_dict, _want_arrays

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "bin", "k-mer-count")
U64, U32 = np.uint64, np.uint32
RANGES = ((1, 0), (2, 0), (1, 1), (2, 3))


def _dev_u32(ptr, n):
    return _dev_bytes(ptr, 4 * n).view(U32)


def _want(lk):
    return np.array(lk.offsets, U64), np.array(lk.to, U32)


def _raw(kmc, kc, lo, hi, nu, nl, spare=3):
    """kmc_unitig_links through ctypes into arrays with `spare` entries more than needed, filled with a pattern"""
    L = kmc.lib()
    offs, to = np.full(2 * nu + 1 + spare, 0xEEEE, U64), np.full(nl + spare, 0xEEEEEEEE, U32)
    n1, n2 = C.c_uint64(12345), C.c_uint64(12345)
    w = (C.c_uint64 * kmc.LINK_WORDS)()
    kc._chk(L.kmc_unitig_links(kc._h, lo, hi, offs.ctypes.data, 2 * nu + spare, to.ctypes.data, nl + spare, C.byref(n1), C.byref(n2), w))
    assert (n1.value, n2.value) == (nu, nl)
    assert (offs[2 * nu + 1:] == 0xEEEE).all() and (to[nl:] == 0xEEEEEEEE).all()
    return (offs[:2 * nu + 1], to[:nl]), list(w)


def _equal(got, want, ctx):
    for name, g, w in zip(("offsets", "to"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (ctx, name, g[:40], w[:40])


def _check(kmc, kc, table, canonical, ranges):
    """every form of the call against the model, for every range; returns {range: the model's Links}"""
    L = kmc.lib()
    seen = {}
    for lo, hi in ranges:
        lk = lm.links(table, canonical, lo, hi)
        want, words = _want(lk), lk.summary
        nu, nl = words[0], words[1]
        ctx = (kc.k, canonical, lo, hi)
        # the sizing call
        n1, n2 = C.c_uint64(1), C.c_uint64(1)
        w = (C.c_uint64 * 8)()
        kc._chk(L.kmc_unitig_links(kc._h, lo, hi, None, 0, None, 0, C.byref(n1), C.byref(n2), w))
        assert (n1.value, n2.value, list(w)) == (nu, nl, words), (ctx, list(w), words)
        got, w = _raw(kmc, kc, lo, hi, nu, nl)
        assert w == words, (ctx, w, words)
        _equal(got, want, ctx)
        # the device form, read back
        do, dt, dn, dl, s = kc.unitig_links_device(lo, hi)
        assert (dn, dl, s.words()) == (nu, nl, words) and do and dt and do % 8 == 0 and dt % 4 == 0
        _equal((_dev_u64(do, 2 * nu + 1), _dev_u32(dt, nl)), want, ctx)
        r = kc.unitig_links(lo, hi)
        _equal((r.offsets, r.to), want, ctx)
        assert r.summary.words() == words and len(r) == nl and list(r.records()) == list(lk.records())
        # the degree identity, on the library's own three summaries
        g, t = kc.graph(lo, hi, adj=False)[1].words(), kc.unitigs(lo, hi).summary.words()
        assert g[1] + g[2] == words[1] + words[5] + 2 * (t[2] - t[0]) and t[0] == words[0], (ctx, g, t, words)
        seen[(lo, hi)] = lk
    return seen


def _check_reads(kmc, oracle, reads, k, canonical, ranges=RANGES):
    bases, offs = _pack(reads)
    want = oracle.count_kmers(bases, offs, k, canonical)
    table = _table_dict(want)
    assert table == gm.count_table(reads, k, canonical)
    with kmc.KmerCounter(k=k, canonical=canonical) as kc:
        kc.add_batch(bases, offs)
        assert kc.export().equals(want)
        return _check(kmc, kc, table, canonical, ranges), table


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [1, 2, 4, 5, 6, 21, 31, 32, 33, 47, 63])
def test_sample_fasta(kmc, oracle, k, canonical):
    bases, offs = kmc.parse_fasta(SAMPLE)
    want = oracle.count_kmers(bases, offs, k, canonical)
    with kmc.KmerCounter(k=k, canonical=canonical) as kc:
        kc.add_batch(bases, offs)
        assert kc.export().equals(want)
        _check(kmc, kc, _table_dict(want), canonical, RANGES + ((20, 0), (3, 6)))   # (no key of the sample is seen twice or less)


def _branching(k, seed, few=False):
    """Reads whose graph still branches at large k: a random sequence of 600 bases tiled by reads of 200 that overlap by
    100; three single-base variants of it, each a read that reaches k + 5 bases to either side (bubbles); a stretch of
    k + 10 bases between different flanks in two places (a repeat); a fork, twice; and the shapes of the unitig test --
    the homopolymer, the AT repeat, circular reads of 100 and of 2 bases (twice each), for even k the palindrome read.
    few: the same shapes in some hundred k-mers -- a sequence of 30 bases with one variant, a repeat between flanks of 4, a
    fork with arms of 5, circular reads of 12 and of 2 bases -- for a k whose k-mer space the full set nearly fills."""
    rng = np.random.default_rng(seed)
    n, flank, arm, circ = (30, 4, 5, 12) if few else (600, 40, 40, 100)
    s = _rnd(rng, n)
    reads = [s] if few else [s[i:i + 200] for i in range(0, 500, 100)]
    for p in ((n // 2,) if few else (150, 300, 450)):
        alt = "ACGT"[("ACGT".index(s[p]) + 1 + int(rng.integers(0, 3))) % 4]
        reads.append(s[max(p - k - 5, 0):p] + alt + s[p + 1:p + k + 6])
    rep = _rnd(rng, k + 10)
    reads += [_rnd(rng, flank) + rep + _rnd(rng, flank), _rnd(rng, flank) + rep + _rnd(rng, flank)]
    stem = _rnd(rng, k + (4 if few else 30))
    reads += [stem + _rnd(rng, arm), stem + _rnd(rng, arm)] * 2
    reads.append("A" * (k + 20))
    reads.append(("AT" * (k + 20))[: k + 31])
    for m in (circ, 2):
        c = _rnd(rng, m)
        reads += [(c * (k + 2))[:m + k + 2]] * 2
    if k % 2 == 0:
        half = _rnd(rng, k // 2)
        reads.append("G" + half + gm.revcomp(half) + "C")
    return reads


def _circular_closes(table, canonical, rng_, lk):
    """a circular unitig whose END end reaches its own START end"""
    u = um.unitigs(table, canonical, *rng_)
    return any(f and 2 * i in lk.to[lk.offsets[2 * i + 1]:lk.offsets[2 * i + 2]] for i, f in enumerate(u.flags))


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [6, 21, 31, 32, 33, 63])
def test_branching_reads(kmc, oracle, k, canonical):
    seen, table = _check_reads(kmc, oracle, _branching(k, 900 + k), k, canonical)
    if k < 21:
        # At k = 6 the full set nearly fills the space of 6-mers and no cycle survives the branching: it checks exactness
        # alone there, and the few reads of the same shapes carry the assertions.
        seen, table = _check_reads(kmc, oracle, _branching(k, 900 + k, few=True), k, canonical)
    words = [lk.summary for lk in seen.values()]
    # the input is what it claims to be (the model's values)
    assert any(w[3] > 0 for w in words) and any(w[2] > 0 for w in words) and any(w[4] > 0 for w in words), words
    assert any(w[7] >= 2 for w in words) and any(w[6] > 0 for w in words), words
    assert any(_circular_closes(table, canonical, r, lk) for r, lk in seen.items())
    if canonical and k % 2 == 0:
        assert any(w[5] > 0 for w in words), words
    else:
        assert all(w[5] == 0 for w in words), words
    if k >= 21:   # the bubbles, the repeat and the fork survive: dozens of records, not the dozen of a few tips
        assert seen[(1, 0)].summary[1] >= 30 and seen[(1, 0)].summary[3] >= 8, words


@pytest.mark.parametrize("canonical", [True, False])
def test_dense_small_k(kmc, oracle, canonical):
    """2000 random bases at k = 5: most of the 5-mer space, hundreds of one-key unitigs, ends with all four bits set"""
    seen, table = _check_reads(kmc, oracle, [_rnd(np.random.default_rng(55), 2000)], 5, canonical)
    w = seen[(1, 0)].summary
    assert w[7] == 4 and w[0] >= 200 and w[3] >= 200, w
    assert um.unitigs(table, canonical).summary[4] >= 200


@pytest.mark.parametrize("k,canonical", [(31, True), (31, False), (63, True)])
def test_table_of_many_workgroups(kmc, oracle, k, canonical):
    """rows, ends and the scan of the per-end counts cross workgroup and scan-block boundaries"""
    n_reads = 640
    sb, so = kmc.synth_reads_host(kmc.Synth(seed=31, pool=0), 0, n_reads)     # 400-base reads, every line fresh random
    # the first 150 reads twice: counts of 2; and off every read a branch -- 100 of its bases, then 40 fresh ones -- so that
    # there are three unitigs and four records per read: more ends and more records than one scan block takes
    rng = np.random.default_rng(31)
    arms = [np.concatenate([sb[int(so[i]) + 100:int(so[i]) + 200], np.frombuffer(_rnd(rng, 40).encode(), np.uint8)]) for i in range(n_reads)]
    bases = np.concatenate([sb, sb[:int(so[150])]] + arms)
    offs = np.concatenate([so, so[1:151] + so[-1], so[-1] + so[150] + 140 * np.arange(1, n_reads + 1, dtype=U64)])
    want = oracle.count_kmers(bases, offs, k, canonical, method=1)
    assert want.n_distinct >= 200_000
    table = _table_dict(want)
    lk = lm.links(table, canonical)      # (one range: the model walks a table of this size for ten seconds)
    assert 2 * lk.summary[0] > 2048 and lk.summary[1] > 2048 and lk.summary[3] >= 600, lk.summary
    with kmc.KmerCounter(k=k, canonical=canonical) as kc:
        kc.add_batch(bases, offs)
        assert kc.export().equals(want)
        got, w = _raw(kmc, kc, 1, 0, lk.summary[0], lk.summary[1])
        assert w == lk.summary
        _equal(got, _want(lk), (k, canonical))
        do, dt, dn, dl, s = kc.unitig_links_device(1, 0)
        assert s.words() == lk.summary
        _equal((_dev_u64(do, 2 * dn + 1), _dev_u32(dt, dl)), _want(lk), (k, canonical, "device"))


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("n_rows", [64, 65, 256, 257])
def test_view_rows_at_the_wave_and_workgroup_seams(kmc, oracle, n_rows, canonical):
    """a view of exactly n_rows keys, branching among its first rows' worth of reads"""
    k = 31
    rng = np.random.default_rng(3000 + n_rows)
    stem = _rnd(rng, k + 3)
    reads = [stem + _rnd(rng, 6), stem + _rnd(rng, 6), "A" * (k + 2)]
    m = len(gm.count_table(reads, k, canonical))
    assert m < n_rows
    reads.append(_rnd(rng, n_rows - m + k - 1))                               # every window of it a new key
    assert len(gm.count_table(reads, k, canonical)) == n_rows
    seen, _ = _check_reads(kmc, oracle, reads, k, canonical, ((1, 0),))
    assert seen[(1, 0)].summary[1] >= 4 and seen[(1, 0)].summary[4] >= 2


_CHILD = r"""
import importlib, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
kmc = importlib.import_module("k-mer-count_amd")
bases, offs = kmc.parse_fasta(sys.argv[2])
with kmc.KmerCounter(k=31) as kc:
    kc.add_batch(bases, offs)
    kc.finalize()
    print("step unitigs(1,0)", file=sys.stderr, flush=True)
    kc.unitigs(1, 0)
    print("step links(1,0)", file=sys.stderr, flush=True)
    a = kc.unitig_links(1, 0)
    print("step links(1,0) again", file=sys.stderr, flush=True)
    b = kc.unitig_links(1, 0)
    assert np.array_equal(a.to, b.to)
    print("step links_device(1,0)", file=sys.stderr, flush=True)
    kc.unitig_links_device(1, 0)
    print("step graph(2,0) links(1,0)", file=sys.stderr, flush=True)
    kc.graph(2, 0, adj=False)
    kc.unitig_links(1, 0)
    print("step links(2,0)", file=sys.stderr, flush=True)
    kc.unitig_links(2, 0)
    print("step end", file=sys.stderr, flush=True)
"""


def test_links_after_unitigs_compute_the_unitigs_once(kmc):
    """What computes, seen through the KMC_UNITIG_TRACE lines of a child process (nothing is timed)"""
    env = dict(os.environ, KMC_UNITIG_TRACE="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, SAMPLE], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    steps, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("step "):
            cur = line[5:]
            steps[cur] = []
        elif line.startswith("kmc_unitigs:") or line.startswith("kmc_unitig_links:"):
            steps[cur].append(line.split(":")[0] + (" reused" if "unitigs_reused 1" in line else ""))
    # unitigs() is a sizing call that computes and a copy call that does not
    assert steps["unitigs(1,0)"] == ["kmc_unitigs"]
    # the links pass alone, once for the two host calls; the host form then copies the kept links
    assert steps["links(1,0)"] == ["kmc_unitig_links reused"]
    assert steps["links(1,0) again"] == []
    # the device form always runs the links pass, on the kept unitigs
    assert steps["links_device(1,0)"] == ["kmc_unitig_links reused"]
    # a graph call with another range has rewritten adj: the host form still copies its kept links ...
    assert steps["graph(2,0) links(1,0)"] == []
    # ... and another range computes both
    assert steps["links(2,0)"] == ["kmc_unitigs", "kmc_unitig_links"]
    assert "links_ms" in r.stderr


def test_reuse_never_serves_a_stale_result(kmc, oracle):
    bases, offs = kmc.parse_fasta(SAMPLE)
    half = len(offs) // 2
    b1, o1 = bases[:int(offs[half])], offs[:half + 1]
    full = _table_dict(oracle.count_kmers(bases, offs, 31, True))
    part = _table_dict(oracle.count_kmers(b1, o1, 31, True))
    want = {(id(t), r): lm.links(t, True, *r) for t in (full, part) for r in ((1, 0), (2, 0))}

    def links_are(kc, table, lo, hi, device=False):
        lk = want[(id(table), (lo, hi))]
        if device:
            do, dt, dn, dl, s = kc.unitig_links_device(lo, hi)
            got, w = (_dev_u64(do, 2 * dn + 1), _dev_u32(dt, dl)), s.words()
        else:
            got, w = _raw(kmc, kc, lo, hi, lk.summary[0], lk.summary[1])
        assert w == lk.summary
        _equal(got, _want(lk), (lo, hi, device))

    def unitigs_are(kc, table, lo, hi):
        u = um.unitigs(table, True, lo, hi)
        r = kc.unitigs(lo, hi)
        _same((r.bases, r.offsets, r.abund, r.flags), _want_arrays(u), (lo, hi))
        assert r.summary.words() == u.summary

    # what a stale answer would be differs from the right one: the two ranges on the first view, the two views at (2, 0)
    assert want[(id(part), (1, 0))].summary != want[(id(part), (2, 0))].summary != want[(id(full), (2, 0))].summary
    first, second = part, full
    for device in (False, True):
        with kmc.KmerCounter(k=31) as kc:
            kc.add_batch(b1, o1)
            kc.finalize()
            # a graph call with another range between the unitigs and their links: adj is that of (2, 0) now
            kc.unitigs(1, 0)
            kc.graph(2, 0)
            links_are(kc, first, 1, 0, device)
            kc.unitigs_device(1, 0)
            kc.graph_device(2, 0)
            links_are(kc, first, 1, 0, device)
            # a links call with another range is followed by the right unitig arrays, and the other way round
            links_are(kc, first, 2, 0, device)
            unitigs_are(kc, first, 2, 0)
            unitigs_are(kc, first, 1, 0)
            links_are(kc, first, 1, 0, device)
            links_are(kc, first, 2, 0, device)
            links_are(kc, first, 2, 0, device)
            # a unitig call of another range between two links calls of one range
            kc.unitigs_device(1, 0)
            links_are(kc, first, 2, 0, device)
            # a finalize in between: the same range on a new view
            kc.reset()
            kc.add_batch(bases, offs)
            kc.finalize()
            links_are(kc, second, 2, 0, device)
            unitigs_are(kc, second, 2, 0)
            links_are(kc, second, 1, 0, device)
            kc.reset()
            kc.finalize()
            r = kc.unitig_links(1, 0)
            assert list(r.offsets) == [0] and len(r) == 0 and r.summary.words() == [0] * 8


def test_after_finalize_async(kmc, oracle):
    hb, ho = kmc.synth_reads_host(kmc.Synth(seed=4), 0, 3000)
    want = oracle.count_kmers(hb, ho, 31, True)
    lk = lm.links(_table_dict(want), True, 2, 0)
    for form in ("unitig_links", "unitig_links_device"):
        with kmc.KmerCounter(k=31) as kc:
            kc.add_batch(hb, ho)
            kc.export()
            kc.reset()
            kc.add_batch(hb, ho)
            ok0 = kc.stats().n_async_ok
            kc.finalize_async()          # a view queued and never observed before the links call
            if form == "unitig_links":
                r = kc.unitig_links(2, 0)
                got, words = (r.offsets, r.to), r.summary.words()
            else:
                do, dt, nu, nl, s = kc.unitig_links_device(2, 0)
                got, words = (_dev_u64(do, 2 * nu + 1), _dev_u32(dt, nl)), s.words()
            _equal(got, _want(lk), form)
            assert words == lk.summary
            assert kc.finalize() == (want.n_distinct, want.n_total)
            assert kc.stats().n_async_ok == ok0 + 1


def test_state_and_errors(kmc, oracle):
    L = kmc.lib()
    bases, offs = kmc.parse_fasta(SAMPLE)
    table = _table_dict(oracle.count_kmers(bases, offs, 31, True))
    n1, n2 = C.c_uint64(99), C.c_uint64(99)
    w = (C.c_uint64 * 8)(*([7] * 8))
    p = [C.c_void_p(1) for _ in range(2)]

    def host(kc, lo, hi):
        return L.kmc_unitig_links(kc._h, lo, hi, None, 0, None, 0, C.byref(n1), C.byref(n2), w)

    def device(kc, lo, hi):
        return L.kmc_unitig_links_device(kc._h, lo, hi, *[C.byref(x) for x in p], C.byref(n1), C.byref(n2), w)

    def state(kc):
        """what the links calls say in this state, checked against kmc_export"""
        rc = L.kmc_export(kc._h, None, None, None, 0)
        exp = kmc.ERR_STATE if rc == kmc.ERR_STATE else kmc.OK
        assert (host(kc, 1, 0) == kmc.ERR_STATE) == (exp == kmc.ERR_STATE)
        assert (device(kc, 1, 0) == kmc.ERR_STATE) == (exp == kmc.ERR_STATE)
        return exp

    assert L.kmc_unitig_links(None, 1, 0, None, 0, None, 0, None, None, None) == kmc.ERR_ARG      # a NULL ctx
    with kmc.KmerCounter(k=31) as kc:
        assert state(kc) == kmc.ERR_STATE                    # before any finalize
        kc.add_batch(bases, offs)
        assert state(kc) == kmc.ERR_STATE
        kc.finalize()
        assert state(kc) == kmc.OK
        # every output pointer may be NULL
        assert L.kmc_unitig_links_device(kc._h, 1, 0, None, None, None, None, None) == kmc.OK
        assert L.kmc_unitig_links(kc._h, 1, 0, None, 0, None, 0, None, None, None) == kmc.OK
        # a bad range
        assert host(kc, 3, 2) == kmc.ERR_ARG and device(kc, 3, 2) == kmc.ERR_ARG
        assert host(kc, 3, 3) == kmc.OK
        lk = lm.links(table, True)
        nu, nl = lk.summary[0], lk.summary[1]
        assert nl > 0
        # the sizing call
        assert host(kc, 1, 0) == kmc.OK and (n1.value, n2.value, list(w)) == (nu, nl, lk.summary)
        # caps one too small: the sizes are set, nothing is copied
        offs_o, to_o = np.full(2 * nu + 1, 0xEEEE, U64), np.full(nl, 0xEEEEEEEE, U32)
        for ce, cl in ((2 * nu - 1, nl), (2 * nu, nl - 1), (0, 0)):
            n1.value = n2.value = 0
            assert L.kmc_unitig_links(kc._h, 1, 0, offs_o.ctypes.data, ce, to_o.ctypes.data, cl, C.byref(n1), C.byref(n2), w) == kmc.ERR_ARG
            assert (n1.value, n2.value) == (nu, nl)
            assert (offs_o == 0xEEEE).all() and (to_o == 0xEEEEEEEE).all()
        # cap_ends counts ends: exactly 2 * n_unitigs is enough for the 2 * n_unitigs + 1 offsets
        assert L.kmc_unitig_links(kc._h, 1, 0, offs_o.ctypes.data, 2 * nu, None, 0, C.byref(n1), C.byref(n2), None) == kmc.OK
        assert np.array_equal(offs_o, np.array(lk.offsets, U64)) and (to_o == 0xEEEEEEEE).all()
        # one array alone: the cap of the one that is NULL is not looked at
        assert L.kmc_unitig_links(kc._h, 1, 0, None, 0, to_o.ctypes.data, nl, None, None, None) == kmc.OK
        assert np.array_equal(to_o, np.array(lk.to, U32))
        kc.reset()
        assert state(kc) == kmc.ERR_STATE
        # an empty view: zeros, offsets[0] == 0
        kc.finalize()
        r = kc.unitig_links()
        assert len(r) == 0 and list(r.offsets) == [0] and r.to.shape == (0,) and r.summary.words() == [0] * 8 and list(r.records()) == []
        d = kc.unitig_links_device()
        assert d[2:4] == (0, 0) and d[4].words() == [0] * 8 and d[0] and list(_dev_u64(d[0], 1)) == [0]
        one = np.full(1, 0xEEEE, U64)
        assert L.kmc_unitig_links(kc._h, 1, 0, one.ctypes.data, 0, None, 0, C.byref(n1), C.byref(n2), w) == kmc.OK and one[0] == 0
    with kmc.KmerCounter(k=31) as kc:     # a range that no key is in
        kc.add_batch(bases, offs)
        kc.finalize()
        r = kc.unitig_links(10 ** 9, 0)
        assert len(r) == 0 and list(r.offsets) == [0] and r.summary.words() == [0] * 8
    with kmc.KmerCounter(mode=kmc.MODE_LR) as kc:
        kc.count_file(SAMPLE)
        kc.finalize()
        assert host(kc, 1, 0) == kmc.ERR_ARG and device(kc, 1, 0) == kmc.ERR_ARG
        with pytest.raises(kmc.KmcError) as e:
            kc.unitig_links()
        assert e.value.status == kmc.ERR_ARG


def test_nothing_else_moved(kmc, oracle):
    bases, offs = kmc.parse_fasta(SAMPLE)
    half = len(offs) // 2
    for k in (31, 63):
        want = oracle.count_kmers(bases, offs, k, True)
        table = _table_dict(want)
        rng = np.random.default_rng(k)
        qlo = np.concatenate([want.key_lo, want.key_lo ^ U64(1)])
        qhi = np.concatenate([want.key_hi, want.key_hi])
        p = rng.permutation(len(qlo))
        qlo, qhi = qlo[p], qhi[p]
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
            arrays = ((plo, n), (pcnt, n), (flo, nk), (fcnt, nk), (slo, ns), (scnt, ns), (do, nu + 1), (da, nu))
            before = [_dev_u64(ptr, m) for ptr, m in arrays] + [_dev_bytes(db, nb), _dev_bytes(df, nu)]
            q_before = kc.query(qlo, qhi)                     # builds the index
            assert q_before.any() and not q_before.all()
            _check(kmc, kc, table, True, ((2, 0),))           # the links of the range whose unitigs the ctx holds
            after = [_dev_u64(ptr, m) for ptr, m in arrays] + [_dev_bytes(db, nb), _dev_bytes(df, nu)]
            assert all(np.array_equal(a, b) for a, b in zip(before, after))
            u = um.unitigs(table, True, 2, 0)
            _same((after[8], after[6], after[7], after[9]), _want_arrays(u), k)
            assert kc.export_device() == vp and kc.export().digest() == digest
            assert np.array_equal(kc.query(qlo, qhi), q_before)
            _check(kmc, kc, table, True, ((1, 0),))
            assert kc.export_device() == vp and kc.export().digest() == digest
            assert np.array_equal(kc.query(qlo, qhi), q_before)
        # the other order: the links call builds the index, the query reuses it
        with kmc.KmerCounter(k=k) as kc:
            kc.add_batch(bases, offs)
            kc.finalize()
            _check(kmc, kc, table, True, ((1, 0),))
            assert np.array_equal(kc.query(qlo, qhi), q_before)


@pytest.mark.parametrize("forward", [False, True])
@pytest.mark.parametrize("k", [31, 63])
def test_cli_gfa(kmc, oracle, k, forward):
    bases, offs = kmc.parse_fasta(SAMPLE)
    table = _table_dict(oracle.count_kmers(bases, offs, k, not forward))
    fw = ["--forward"] if forward else []
    for rng_args, (lo, hi) in (([], (1, 0)), (["--min-count", "2"], (2, 0))):
        r = subprocess.run([EXE, SAMPLE, "-k", str(k), "--gfa"] + rng_args + fw, capture_output=True, text=True)
        want = lm.gfa(um.unitigs(table, not forward, lo, hi), lm.links(table, not forward, lo, hi), k)
        assert r.returncode == 0 and r.stdout == want, r.stderr
        assert want.count("\nL\t") > 0
    # the Python writer prints the same text
    with kmc.KmerCounter(k=k, canonical=not forward) as kc:
        kc.add_batch(bases, offs)
        kc.finalize()
        assert kc.unitigs(2, 0).to_gfa(kc.unitig_links(2, 0), k) == want
