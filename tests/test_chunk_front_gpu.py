"""The seam batch of tests/chunk_inputs.py through every kernel behind the chunk front end (kmc_chunks.hip.h): counting with
KMC_ALGO_STREAM and KMC_ALGO_SORT against the oracle, kmc_profile against the walker of tests/test_query_gpu.py,
kmc_unitig_map against tests/map_model.py.  The batch is counted into the table it is profiled and mapped on."""
import numpy as np
import pytest

import chunk_inputs as ci
import map_model as mm
from test_map_gpu import _device, _equal, _want
from test_query_gpu import _sat32, _table_dict, _walk

pytestmark = pytest.mark.gpu

KS = (5, 31, 32, 33, 63)
_cache = {}


def _seam(oracle, k, canonical):
    """(bases, offsets, the oracle's table of the batch), computed once per case and left unchanged"""
    key = (k, canonical)
    if key not in _cache:
        bases, offs = ci.seam_batch(k)
        bases.setflags(write=False)
        offs.setflags(write=False)
        _cache[key] = (bases, offs, oracle.count_kmers(bases, offs, k, canonical))
    return _cache[key]


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", KS)
def test_seam_batch_counted(kmc, oracle, k, canonical):
    bases, offs, want = _seam(oracle, k, canonical)
    assert int(want.count.max()) > 1
    for algo in (kmc.ALGO_STREAM, kmc.ALGO_SORT):
        with kmc.KmerCounter(k=k, canonical=canonical, algo=algo) as kc:
            kc.add_batch(bases, offs)
            got, st = kc.export(), kc.stats()
        assert st.algo_last == algo, (k, canonical, algo, st.algo_last)
        assert got.equals(want), (k, canonical, algo, got.n_distinct, want.n_distinct, got.n_total, want.n_total)


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", KS)
def test_seam_batch_profiled(kmc, oracle, k, canonical):
    bases, offs, want = _seam(oracle, k, canonical)
    table = _table_dict(want)
    with kmc.KmerCounter(k=k, canonical=canonical) as kc:
        kc.add_batch(bases, offs)
        kc.finalize()
        for min_count in (1, 2):
            mw, ms = _walk(bases, offs, k, canonical, table, min_count)
            win, rs = kc.profile(bases, offs, min_count)
            bad = np.nonzero(win != _sat32(mw))[0]
            assert not len(bad), (k, canonical, bad[:10], win[bad[:10]], [mw[i] for i in bad[:10]])
            badr = np.nonzero((rs != ms).any(axis=1))[0]
            assert not len(badr), (k, canonical, min_count, badr[:5], rs[badr[:5]], ms[badr[:5]])


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", KS)
def test_seam_batch_mapped(kmc, oracle, k, canonical):
    bases, offs, want = _seam(oracle, k, canonical)
    table = {kmer.decode(): c for kmer, c in _table_dict(want).items()}
    m = mm.map_reads(table, canonical, ci.reads_of(bases, offs), 1, 0, k=k)
    arrays, words = _want(m), m.summary
    assert words[2] > 0, words
    with kmc.KmerCounter(k=k, canonical=canonical) as kc:
        kc.add_batch(bases, offs)
        kc.finalize()
        r = kc.map_reads(bases, offs, 1, 0)
        _equal((r.place, r.stats, r.seg_offsets, r.segments, r.support), arrays, (k, canonical, "map_reads"))
        assert r.summary.words() == words, (k, canonical, r.summary.words(), words)
        got, ns, nu, w = _device(kc, 1, 0, bases, offs)
        assert (ns, nu, w) == (words[3], m.n_unitigs, words), (k, canonical, ns, nu, w, words)
        _equal(got, arrays, (k, canonical, "device"))
