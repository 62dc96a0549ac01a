"""GPU checks of kmc_graph / kmc_graph_device / KmerCounter.graph (kmc_graph.hip.h).  Expected values come from
tests/graph_model.py -- the definition in its neighbour form, on Python strings -- applied to the CPU oracle's table of the
same input.  All comparisons are exact."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import graph_model as gm
from conftest import ROOT, SAMPLE

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "bin", "k-mer-count")
U64 = np.uint64
RANGES = ((1, 0), (2, 0), (1, 1), (2, 3))


def _table_dict(t):
    """{k-mer string: count} of an oracle table."""
    km = t.kmers()
    return {km[i].tobytes().decode(): int(t.count[i]) for i in range(t.n_distinct)}


def _pack(reads):
    bases = np.frombuffer("".join(reads).encode(), np.uint8)
    offs = np.zeros(len(reads) + 1, U64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return bases, offs


def _dev_u16(ptr, n):
    """n uint16 at a device address (read as whole 64-bit words: the ctx's arrays are allocated with room to spare)"""
    kd = importlib.import_module("k-mer-count_amd.distributed")
    import torch
    return kd.device_view(ptr, (2 * n + 7) // 8, torch.device("cuda", 0)).cpu().numpy().view(np.uint16)[:n].copy()


def _raw_graph(kmc, kc, lo, hi, n_view, spare=3):
    """kmc_graph through ctypes into an array with `spare` entries more than needed: (adj, the spare tail, n_keys, words)"""
    L = kmc.lib()
    out = np.full(n_view + spare, 0xFFFF, np.uint16)
    n = C.c_uint64(12345)
    w = (C.c_uint64 * kmc.GRAPH_WORDS)()
    kc._chk(L.kmc_graph(kc._h, lo, hi, out.ctypes.data, len(out), C.byref(n), w))
    return out[:n_view], out[n_view:], n.value, list(w)


def _check(kmc, kc, table, canonical, ranges=RANGES):
    """every form of the call against the model, for every range; returns {range: model words}"""
    seen = {}
    for lo, hi in ranges:
        keys, adj, words = gm.graph(table, canonical, lo, hi)
        want = np.array(adj, np.uint16)
        got, tail, n, w = _raw_graph(kmc, kc, lo, hi, len(keys))
        bad = np.nonzero(got != want)[0]
        assert n == len(keys) and not len(bad), (kc.k, canonical, lo, hi, n, len(keys), bad[:8], got[bad[:8]], want[bad[:8]],
                                                 [keys[i] for i in bad[:8]])
        assert (tail == 0xFFFF).all()
        assert w == words, (kc.k, canonical, lo, hi, w, words)
        ptr, nd, s = kc.graph_device(lo, hi)
        assert nd == len(keys) and s.words() == words and (ptr or not nd)
        assert np.array_equal(_dev_u16(ptr, nd), want)
        a, s = kc.graph(lo, hi)
        assert a.dtype == np.uint16 and np.array_equal(a, want) and s.words() == words and s.unitigs == words[6] // 2
        none, s = kc.graph(lo, hi, adj=False)
        assert none is None and s.words() == words
        seen[(lo, hi)] = words
    return seen


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [1, 2, 4, 5, 6, 21, 31, 32, 33, 47, 63])
def test_sample_fasta(kmc, oracle, k, canonical):
    bases, offs = kmc.parse_fasta(SAMPLE)
    want = oracle.count_kmers(bases, offs, k, canonical)
    table = _table_dict(want)
    with kmc.KmerCounter(k=k, canonical=canonical) as kc:
        kc.add_batch(bases, offs)
        assert kc.export().equals(want)
        seen = _check(kmc, kc, table, canonical, ((1, 0), (2, 0), (3, 6), (1, 2)))
    if k == 31 and canonical:   # the anchor: branching and ends, but no isolated node and no dead end in this input
        assert seen[(1, 0)] == [3260, 3346, 3354, 0, 0, 140, 460, 70]


def _rnd(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def _constructed(k, seed):
    """Random reads of lengths k, k + 1, k + 5, 150 and 400, each one to three times; a fork (two reads sharing a 150-base
    prefix, twice, so that it stays solid at min_count 2); a read with an N; the other strand of a stretch of a long read;
    a homopolymer; an AT repeat."""
    rng = np.random.default_rng(seed)
    reads = []
    for n in (k, k + 1, k + 5, 150, 400):
        for _ in range(6):
            reads += [_rnd(rng, max(n, k))] * int(rng.integers(1, 4))
    stem = _rnd(rng, 150)
    reads += [stem + _rnd(rng, 60), stem + _rnd(rng, 60)] * 2
    s = _rnd(rng, 200)
    reads.append(s[:90] + "N" + s[91:])
    long_ = [r for r in reads if len(r) == 400][0]
    reads.append(gm.revcomp(long_[100:300]))
    reads.append("A" * (k + 20))
    reads.append(("AT" * (k + 20))[: k + 31])
    return reads


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [6, 21, 31, 32, 33, 63])
def test_constructed_reads_cover_every_summary_word(kmc, oracle, k, canonical):
    reads = _constructed(k, 500 + k)
    bases, offs = _pack(reads)
    want = oracle.count_kmers(bases, offs, k, canonical)
    table = _table_dict(want)
    assert table == gm.count_table(reads, k, canonical)
    with kmc.KmerCounter(k=k, canonical=canonical) as kc:
        kc.add_batch(bases, offs)
        assert kc.export().equals(want)
        seen = _check(kmc, kc, table, canonical)
    # what makes this input worth having: a range in which isolated nodes, dead ends, branching nodes and single-node
    # unitigs all occur, and a range in which part of the view is not solid
    assert any(all(w) for w in seen.values()), seen
    assert any(w[0] < len(table) for w in seen.values()), seen


@pytest.mark.parametrize("k", [31, 63])
def test_table_of_many_workgroups(kmc, oracle, k):
    n_reads = 640
    sb, so = kmc.synth_reads_host(kmc.Synth(seed=31, pool=0), 0, n_reads)     # 400-base reads, every line fresh random
    bases = np.concatenate([sb, sb[:int(so[150])]])                            # the first 150 reads twice: counts of 2
    offs = np.concatenate([so, so[1:151] + so[-1]])
    for canonical in ((True, False) if k == 31 else (True,)):
        want = oracle.count_kmers(bases, offs, k, canonical, method=1)
        assert want.n_distinct >= 200_000
        table = _table_dict(want)
        with kmc.KmerCounter(k=k, canonical=canonical) as kc:
            kc.add_batch(bases, offs)
            assert kc.export().equals(want)
            seen = _check(kmc, kc, table, canonical, ((1, 0), (2, 0)))
        assert seen[(1, 0)][0] == want.n_distinct and 0 < seen[(2, 0)][0] < want.n_distinct


def test_state_and_errors(kmc, oracle):
    L = kmc.lib()
    bases, offs = kmc.parse_fasta(SAMPLE)
    half = len(offs) // 2
    b1, o1 = bases[:int(offs[half])], offs[:half + 1]
    t1 = _table_dict(oracle.count_kmers(b1, o1, 31, True))
    t2 = _table_dict(oracle.count_kmers(bases, offs, 31, True))
    n = C.c_uint64(99)
    w = (C.c_uint64 * 8)(*([7] * 8))
    p = C.c_void_p(1)

    def state(kc):
        """what the graph calls say in this state, checked against kmc_export"""
        rc = L.kmc_export(kc._h, None, None, None, 0)
        exp = kmc.ERR_STATE if rc == kmc.ERR_STATE else kmc.OK
        assert (L.kmc_graph(kc._h, 1, 0, None, 0, C.byref(n), w) == kmc.ERR_STATE) == (exp == kmc.ERR_STATE)
        assert (L.kmc_graph_device(kc._h, 1, 0, C.byref(p), C.byref(n), w) == kmc.ERR_STATE) == (exp == kmc.ERR_STATE)
        return exp

    with kmc.KmerCounter(k=31) as kc:
        assert state(kc) == kmc.ERR_STATE                    # before any finalize
        kc.add_batch(b1, o1)
        assert state(kc) == kmc.ERR_STATE
        kc.finalize()
        assert state(kc) == kmc.OK
        # every output pointer may be NULL
        assert L.kmc_graph_device(kc._h, 1, 0, None, None, None) == kmc.OK
        assert L.kmc_graph(kc._h, 1, 0, None, 0, None, None) == kmc.OK
        # a bad range
        assert L.kmc_graph(kc._h, 3, 2, None, 0, C.byref(n), w) == kmc.ERR_ARG
        assert L.kmc_graph_device(kc._h, 3, 2, C.byref(p), C.byref(n), w) == kmc.ERR_ARG
        assert L.kmc_graph(kc._h, 3, 3, None, 0, C.byref(n), w) == kmc.OK and n.value == len(t1)
        # too small: *n_keys is set, nothing is copied
        out = np.full(len(t1), 0xFFFF, np.uint16)
        n.value = 0
        assert L.kmc_graph(kc._h, 1, 0, out.ctypes.data, len(t1) - 1, C.byref(n), w) == kmc.ERR_ARG
        assert n.value == len(t1) and (out == 0xFFFF).all()
        assert L.kmc_graph(kc._h, 1, 0, None, len(t1), C.byref(n), w) == kmc.ERR_ARG        # room claimed, no array
        _check(kmc, kc, t1, True, ((1, 0),))
        # more batches, a second finalize: the new graph, not the old index or buffer
        kc.add_batch(bases[int(offs[half]):], offs[half:] - offs[half])
        assert state(kc) == kmc.ERR_STATE                    # the view is stale
        kc.finalize()
        _check(kmc, kc, t2, True, ((1, 0), (2, 0)))
        kc.reset()
        assert state(kc) == kmc.ERR_STATE
        # an empty view: zeros
        kc.finalize()
        a, s = kc.graph()
        assert a.shape == (0,) and s.words() == [0] * 8
        ptr, nd, s = kc.graph_device()
        assert nd == 0 and s.words() == [0] * 8
    with kmc.KmerCounter(k=31) as kc:     # reads shorter than k: an empty view too
        kc.add_batch(*_pack(["ACGTACGT", "TTTT", "A" * 30]))
        kc.finalize()
        n.value = 5
        assert L.kmc_graph(kc._h, 1, 0, None, 0, C.byref(n), w) == kmc.OK and n.value == 0 and list(w) == [0] * 8
    with kmc.KmerCounter(mode=kmc.MODE_LR) as kc:
        kc.count_file(SAMPLE)
        kc.finalize()
        assert L.kmc_graph(kc._h, 1, 0, None, 0, C.byref(n), w) == kmc.ERR_ARG
        assert L.kmc_graph_device(kc._h, 1, 0, C.byref(p), C.byref(n), w) == kmc.ERR_ARG
        with pytest.raises(kmc.KmcError) as e:
            kc.graph()
        assert e.value.status == kmc.ERR_ARG


def test_after_finalize_async(kmc, oracle):
    hb, ho = kmc.synth_reads_host(kmc.Synth(seed=4), 0, 3000)
    want = oracle.count_kmers(hb, ho, 31, True)
    table = _table_dict(want)
    _, adj, words = gm.graph(table, True, 2, 0)
    with kmc.KmerCounter(k=31) as kc:
        kc.add_batch(hb, ho)
        kc.finalize()
        sync_adj, sync_s = kc.graph(2, 0)
    assert np.array_equal(sync_adj, np.array(adj, np.uint16)) and sync_s.words() == words
    for form in ("graph", "graph_device"):
        with kmc.KmerCounter(k=31) as kc:
            kc.add_batch(hb, ho)
            kc.export()
            kc.reset()
            kc.add_batch(hb, ho)
            ok0 = kc.stats().n_async_ok
            kc.finalize_async()          # a view queued and never observed before the graph call
            if form == "graph":
                a, s = kc.graph(2, 0)
            else:
                ptr, nd, s = kc.graph_device(2, 0)
                a = _dev_u16(ptr, nd)
            assert np.array_equal(a, sync_adj) and s == sync_s
            assert kc.finalize() == (want.n_distinct, want.n_total)
            assert kc.stats().n_async_ok == ok0 + 1


def _dev_u64(ptr, n):
    kd = importlib.import_module("k-mer-count_amd.distributed")
    import torch
    return kd.device_view(ptr, n, torch.device("cuda", 0)).cpu().numpy().view(U64).copy()


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
            arrays = ((plo, n), (pcnt, n), (flo, nk), (fcnt, nk), (slo, ns), (scnt, ns))
            before = [_dev_u64(ptr, m) for ptr, m in arrays]
            q_before = kc.query(qlo, qhi)                     # builds the index
            assert q_before.any() and not q_before.all()
            _check(kmc, kc, table, True, ((1, 0), (2, 0)))    # reuses it
            after = [_dev_u64(ptr, m) for ptr, m in arrays]
            assert all(np.array_equal(a, b) for a, b in zip(before, after))
            assert kc.export_device() == vp and kc.export().digest() == digest
            assert np.array_equal(kc.query(qlo, qhi), q_before)
        # the other order: the graph call builds the index, the query reuses it
        with kmc.KmerCounter(k=k) as kc:
            kc.add_batch(bases, offs)
            kc.finalize()
            _check(kmc, kc, table, True, ((1, 0),))
            assert np.array_equal(kc.query(qlo, qhi), q_before)
            _check(kmc, kc, table, True, ((2, 3),))
            # counting goes on as before
            kc.add_batch(bases, offs)
            t = kc.export()
            assert np.array_equal(t.key_lo, want.key_lo) and np.array_equal(t.count, want.count * U64(2))
            _check(kmc, kc, {x: 2 * c for x, c in table.items()}, True, ((1, 0), (1, 5)))


@pytest.mark.parametrize("forward", [False, True])
@pytest.mark.parametrize("k", [31, 63])
def test_cli_graph(kmc, oracle, k, forward):
    bases, offs = kmc.parse_fasta(SAMPLE)
    table = _table_dict(oracle.count_kmers(bases, offs, k, not forward))
    fw = ["--forward"] if forward else []
    for rng_args, (lo, hi) in (([], (1, 0)), (["--min-count", "3"], (3, 0)), (["--min-count", "2", "--max-count", "4"], (2, 4))):
        r = subprocess.run([EXE, SAMPLE, "-k", str(k), "--graph"] + rng_args + fw, capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout == gm.graph_text(table, not forward, lo, hi), r.stderr
        r = subprocess.run([EXE, SAMPLE, "-k", str(k), "--graph-stats"] + rng_args + fw, capture_output=True, text=True)
        words = gm.graph(table, not forward, lo, hi)[2]
        assert r.returncode == 0 and r.stdout == gm.stats_text(words) == kmc.GraphSummary.from_words(words).to_text(), r.stderr
