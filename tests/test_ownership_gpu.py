"""Every device and pinned allocation of the library is owned by a type that frees it (kmc_mem.hip.h), and the one place
that calls the allocator counts what it does (kmc_debug_mem).  One fresh child process -- its counters start at zero and no
other test's contexts are alive in it -- goes through every call family on small inputs, checks every result against the
oracle or the models of the suite, and ends with every ctx closed: live device bytes, live pinned bytes and failed frees
are then exactly 0.  The out-of-memory paths are not run (nothing here allocates to make an allocation fail).

The child is this file run as a script."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, SAMPLE

pytestmark = pytest.mark.gpu

U64 = np.uint64
# the child: a fresh interpreter that imports torch, opens the GPU, loads the library and runs the sections (a few
# seconds); at the limit it is killed and the test fails
CHILD_LIMIT_S = 120


def _cut(bases, offs, r0, r1):
    return bases[int(offs[r0]):int(offs[r1])], offs[r0:r1 + 1] - offs[r0]


class _Child:
    def __init__(self):
        import importlib
        import oracle_py
        self.kmc = importlib.import_module("k-mer-count_amd")
        self.kmc.lib()
        self.oracle = oracle_py
        oracle_py.lib()
        self.bases, self.offs = oracle_py.parse_fasta(SAMPLE)
        self.n_reads = len(self.offs) - 1
        self.synth = self.kmc.synth_reads_host(self.kmc.Synth(seed=3), 0, 2000)

    def mem(self):
        return self.kmc.debug_mem()

    def open_ctx(self, **kw):
        before = self.mem()
        kc = self.kmc.KmerCounter(**kw)
        m = self.mem()
        # the counter is wired to the real allocator: a ctx cannot be created without device and pinned memory
        assert m[0] > before[0] and m[1] > before[1] and m[2] > before[2] and m[3] > before[3] and m[4] == 0, (before, m)
        return kc

    # ---- what a finalized contiguous-k-mer ctx answers, against the oracle's table `want` of the same input ----
    def check_view(self, kc, want, canonical=True, graph=True):
        import partition_np as P
        from test_graph_gpu import _table_dict
        from test_spectrum_gpu import _np_hist
        from test_unitig_gpu import _dev_u64
        kmc, k = self.kmc, kc.k
        assert kc.finalize() == (want.n_distinct, want.n_total)
        assert kc.export().equals(want)
        h, mx = kc.histogram(101, return_max=True)
        wh, wmx = _np_hist(want.count, 101)
        assert np.array_equal(h, wh) and mx == wmx
        f = kc.export_filtered(2)
        m = want.count >= 2
        assert f.equals(kmc.Table(want.key_hi[m], want.key_lo[m], want.count[m], k))
        # present keys, and neighbours of present keys (absent unless the table happens to hold them)
        qhi = np.concatenate([want.key_hi, want.key_hi])
        qlo = np.concatenate([want.key_lo, want.key_lo ^ U64(1)])
        have = {(int(a), int(b)): int(c) for a, b, c in zip(want.key_hi, want.key_lo, want.count)}
        wq = np.array([have.get((int(a), int(b)), 0) for a, b in zip(qhi, qlo)], U64)
        assert np.array_equal(kc.query(qlo, qhi if k > 31 else None), wq)
        pb, dhi, dlo, dcnt = kc.partition_device(3)
        n = pb[-1]
        P.check_partition(pb, _dev_u64(dhi, n) if k > 31 else np.zeros(n, U64), _dev_u64(dlo, n), _dev_u64(dcnt, n),
                          want.key_hi, want.key_lo, want.count, 3)
        if graph:
            self.check_graph(kc, _table_dict(want), canonical)

    def check_profile(self, kc, want, canonical=True):
        from test_query_gpu import _sat32, _table_dict, _walk
        pb, po = _cut(self.bases, self.offs, 0, 5)
        mw, ms = _walk(pb, po, kc.k, canonical, _table_dict(want), 2)
        win, rs = kc.profile(pb, po, 2)
        assert np.array_equal(win, _sat32(mw)) and np.array_equal(rs, ms)

    def check_graph(self, kc, table, canonical):
        """graph, unitigs, links and the clean pass against their models (range 1..inf and 2..inf: the second one makes every
        stage drop what it holds)"""
        import clean_model as cm
        import graph_model as gm
        import links_model as lm
        import unitig_model as um
        from test_clean_gpu import _equal, _want
        from test_unitig_gpu import _same, _want_arrays
        k = kc.k
        for lo, hi in ((1, 0), (2, 0)):
            keys, adj, words = gm.graph(table, canonical, lo, hi)
            a, s = kc.graph(lo, hi)
            assert np.array_equal(a, np.array(adj, np.uint16)) and s.words() == words
            u, lk = um.unitigs(table, canonical, lo, hi), lm.links(table, canonical, lo, hi)
            r = kc.unitigs(lo, hi)
            _same((r.bases, r.offsets, r.abund, r.flags), _want_arrays(u), (k, lo, hi))
            assert r.summary.words() == u.summary
            l = kc.unitig_links(lo, hi)
            assert np.array_equal(l.offsets, np.array(lk.offsets, U64)) and np.array_equal(l.to, np.array(lk.to, np.uint32))
            assert l.summary.words() == lk.summary
            c = cm.clean(table, canonical, lo, hi, k, k, graph=(u, lk))
            g = kc.clean_unitigs(lo, hi, k, k)
            _equal((g.table.key_hi, g.table.key_lo, g.table.count, g.verdict), _want(self.kmc, c), (k, lo, hi))
            assert g.summary.words() == c.summary
            # a graph call in between rewrites adj: the unitigs the ctx holds lose their work arrays, the links are computed anew
            kc.graph(lo, hi, adj=False)
            l2 = kc.unitig_links(lo, hi)
            assert np.array_equal(l2.to, l.to) and l2.summary.words() == lk.summary

    def check_two_tables(self, ka, kb, a, b):
        import setops_np as M
        assert ka.compare(kb).words() == M.summary(M.of(a), M.of(b))
        assert ka.compare(kb, 2, 0, 1, 3).words() == M.summary(M.of(a), M.of(b), 2, 0, 1, 3)
        for op, mode in ((M.INTERSECT, M.MIN), (M.UNION, M.SUM), (M.SUBTRACT, M.LEFT)):
            (whi, wlo, wc), _ = M.setop(M.of(a), M.of(b), op, mode)
            t = ka.setop(kb, op, mode)
            assert np.array_equal(t.key_hi, whi) and np.array_equal(t.key_lo, wlo) and np.array_equal(t.count, wc), (op, mode)

    def check_clean_into(self, src, dst, table, canonical=True):
        import clean_model as cm
        from test_graph_gpu import _table_dict
        c = cm.clean(table, canonical)
        assert src.clean_into(dst).words() == c.summary
        assert _table_dict(dst.export()) == c.kept

    # ---- the sections ----
    def one_word_keys(self):
        """a: k = 31, canonical, ALGO_WALK, every call family; a second ctx for the two-table calls, a third for clean_into;
        then reset and another input"""
        from test_graph_gpu import _table_dict
        kmc, k = self.kmc, 31
        want = self.oracle.count_kmers(self.bases, self.offs, k, True)
        half = _cut(self.bases, self.offs, 0, self.n_reads // 2)
        want_half = self.oracle.count_kmers(*half, k, True)
        with self.open_ctx(k=k, algo=kmc.ALGO_WALK) as kc:
            kc.add_batch(self.bases, self.offs)
            self.check_view(kc, want)
            self.check_profile(kc, want)
            with self.open_ctx(k=k, algo=kmc.ALGO_WALK) as other:
                other.add_batch(*half)
                other.finalize()
                self.check_two_tables(kc, other, want, want_half)
            with self.open_ctx(k=k) as dst:
                self.check_clean_into(kc, dst, _table_dict(want))
            kc.reset()
            assert kc.finalize() == (0, 0)
            kc.reset()
            kc.add_batch(*self.synth)
            self.check_view(kc, self.oracle.count_kmers(*self.synth, k, True), graph=False)

    def two_word_keys(self):
        """b: k = 63, ALGO_SORT (the hi arrays, runs, the run pool, the merged view), the same calls in brief; count_file and
        count_file_multi (the pinned staging blocks)"""
        from test_graph_gpu import _table_dict
        kmc, k = self.kmc, 63
        want = self.oracle.count_kmers(self.bases, self.offs, k, True)
        third = self.n_reads // 3
        with self.open_ctx(k=k, algo=kmc.ALGO_SORT) as kc:
            kc.add_batch(self.bases, self.offs)
            self.check_view(kc, want)
            self.check_profile(kc, want)
            with self.open_ctx(k=k, algo=kmc.ALGO_SORT) as other:
                cut = _cut(self.bases, self.offs, third, self.n_reads)
                other.add_batch(*cut)
                other.finalize()
                self.check_two_tables(kc, other, want, self.oracle.count_kmers(*cut, k, True))
            with self.open_ctx(k=k) as dst:
                self.check_clean_into(kc, dst, _table_dict(want))
            # table entries (merged pairs) beside a sorted run: the finalize merges them into a view that is a run of its own;
            # the second round hands that view and the runs back to the pool and takes its buffers from there
            import torch
            head = self.oracle.count_kmers(*_cut(self.bases, self.offs, 0, 3), k, True)
            d = [torch.tensor(a.view(np.int64), device="cuda") for a in (head.key_hi, head.key_lo, head.count)]
            torch.cuda.synchronize()
            both = self.oracle.count_kmers(np.concatenate([self.bases, self.bases[:int(self.offs[3])]]),
                                           np.concatenate([self.offs, self.offs[-1] + self.offs[1:4]]), k, True)
            for _ in range(2):
                kc.reset()
                kc.add_batch(self.bases, self.offs)
                kc.merge_pairs_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), head.n_distinct)
                assert kc.finalize() == (both.n_distinct, both.n_total)
                assert kc.export().equals(both)
            kc.reset()
            assert kc.count_file(SAMPLE) == (want.n_distinct, want.n_total)
            assert kc.export().equals(want)
        os.environ["KMC_INGEST_CHUNK_BYTES"] = "9000"       # ten chunks: both pinned blocks of every ctx are used
        try:
            for algo in (kmc.ALGO_AUTO, kmc.ALGO_SORT):
                cs = [self.open_ctx(k=k, algo=algo) for _ in range(2)]
                try:
                    assert kmc.count_file_multi(cs, SAMPLE) == (want.n_distinct, want.n_total)
                    assert cs[0].export().equals(want)
                finally:
                    for c in cs:
                        c.close()
            with self.open_ctx(k=k) as kc:
                assert kc.count_file(SAMPLE) == (want.n_distinct, want.n_total)
                assert kc.export().equals(want)
        finally:
            del os.environ["KMC_INGEST_CHUNK_BYTES"]

    def lr_mode(self):
        """c: the reference's own computation, one batch"""
        cut = _cut(self.bases, self.offs, 0, 40)
        want = self.oracle.count_lr(*cut)
        with self.open_ctx(mode=self.kmc.MODE_LR) as kc:
            kc.add_batch(*cut)
            assert kc.finalize() == (want.n_distinct, want.n_total)
            assert kc.export().equals(want)

    def table_growth(self):
        """d: more distinct keys than half of the initial 2^20 slots: the table is re-allocated and moved into place"""
        k = 31
        rng = np.random.default_rng(31)
        bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 600_000)]
        offs = np.array([0, len(bases)], U64)
        want = self.oracle.count_kmers(bases, offs, k, True, method=1)
        assert want.n_distinct > (1 << 19)
        with self.open_ctx(k=k, capacity_hint=0, algo=self.kmc.ALGO_STREAM) as kc:
            cap0 = int(kc.stats().table_capacity)
            live0 = self.mem()[0]
            assert cap0 == 1 << 20
            kc.add_batch(bases, offs)
            assert kc.finalize() == (want.n_distinct, want.n_total)
            cap1 = int(kc.stats().table_capacity)
            assert cap1 > cap0 and cap1 >= 2 * want.n_distinct, (cap0, cap1)
            assert self.mem()[0] > live0
            assert kc.export().equals(want)

    def error_path(self):
        """e: a byte outside ACGT in reference mode is an error; the ctx closes as any other"""
        kmc = self.kmc
        bases, offs = _cut(self.bases, self.offs, 0, 10)
        bases = bases.copy()
        bases[len(bases) // 2] = ord("N")
        with self.open_ctx(mode=kmc.MODE_LR) as kc:
            with pytest.raises(kmc.KmcError) as e:
                kc.add_batch(bases, offs)
                kc.finalize()
            assert e.value.status == kmc.ERR_ALPHABET

    def stand_alone_calls(self):
        """f: the temporaries of kmc_synth_reads_device and kmc_read_peak_device are gone when the calls return"""
        import torch
        kmc = self.kmc
        s = kmc.Synth(seed=3)
        hb, ho = self.synth
        d_b = torch.zeros(len(hb) + 64, dtype=torch.uint8, device="cuda")
        d_o = torch.zeros(len(ho), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        before = self.mem()
        kmc.synth_reads_device(s, 0, 2000, d_b.data_ptr(), d_o.data_ptr())
        after = self.mem()
        assert after[0] == before[0] and after[1] == before[1] and after[2] == before[2] + 1 and after[4] == 0, (before, after)
        assert np.array_equal(d_b.cpu().numpy()[:len(hb)], hb) and np.array_equal(d_o.cpu().numpy().view(U64), ho)
        n_bytes = len(hb) // 16 * 16
        before = self.mem()
        ms, x = kmc.read_peak_device(d_b.data_ptr(), n_bytes, iters=2)
        after = self.mem()
        assert after[0] == before[0] and after[1] == before[1] and after[2] == before[2] + 1 and after[4] == 0, (before, after)
        # (three launches: the xor of the buffer's 64-bit words, its halves swapped -- kmc_peak.hip.h)
        w = int(np.bitwise_xor.reduce(hb[:n_bytes].view(U64)))
        assert ms > 0 and x == ((w << 32) | (w >> 32)) & 0xFFFFFFFFFFFFFFFF

    def run(self):
        assert self.mem() == (0, 0, 0, 0, 0), self.mem()
        for section in (self.one_word_keys, self.two_word_keys, self.lr_mode, self.table_growth, self.error_path, self.stand_alone_calls):
            section()
            m = self.mem()
            print("after %s: live device %d pinned %d, calls %d / %d, failed frees %d" % ((section.__name__,) + m), flush=True)
            # every ctx of the section is closed: nothing is left, and nothing was freed twice
            assert m[0] == 0 and m[1] == 0 and m[4] == 0, (section.__name__, m)
        m = self.mem()
        assert m[0] == 0 and m[1] == 0 and m[4] == 0 and m[2] > 0 and m[3] > 0, m
        print("ownership child: ok", flush=True)


def test_every_allocation_is_freed_when_its_owner_goes(kmc, oracle):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=CHILD_LIMIT_S, cwd=ROOT)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.rstrip().endswith("ownership child: ok"), r.stdout[-2000:]


if __name__ == "__main__":
    _Child().run()
