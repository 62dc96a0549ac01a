"""Every call ordering around kmc_finalize_async, against the CPU oracle.

kmc_finalize_async queues the small-table finalize and returns; the kernel drains the table into the sorted view and
publishes its outcome to the host.  Whatever call comes next -- an addition of any kind, a reset, a look at the view --
must take that outcome into account (include/kmc.h, kmc_finalize_async).  Adding behind an unobserved finalize used to
lose the first batch's counts (a counter poll overwrote the published outcome), and a reset behind one let the
kernel's late publication stand in for the empty table's counters.  Tables of pairs merged with
kmc_merge_pairs_device are folded into the oracle's table with numpy (slab_np.merge_sorted)."""
import os

import numpy as np
import pytest

import slab_np
from test_spectrum_gpu import _dev_u64, _np_hist, _np_mask

pytestmark = pytest.mark.gpu

SMALL_MAX = 131072   # KMC_FIN_KERNEL_MAX: the largest table the queued finalize takes


def _torch():
    return pytest.importorskip("torch")


def _empty(klen):
    z = np.zeros(0, np.uint64)
    return z, z.copy(), z.copy(), klen


class _Model:
    """Everything added to a ctx since its last reset: reads (oracle) + merged pairs (numpy)."""

    def __init__(self, kmc, oracle, k, canonical, lr=False):
        self.kmc, self.oracle, self.k, self.canonical, self.lr = kmc, oracle, k, canonical, lr
        self.klen = 54 if lr else k
        self.reset()

    def reset(self):
        self.b, self.o, self.pairs, self.n_reads, self._want = [], [np.zeros(1, np.uint64)], [], 0, None

    def add_reads(self, hb, ho):
        self.b.append(hb)
        self.o.append(np.asarray(ho[1:], np.uint64) + self.o[-1][-1])
        self.n_reads += len(ho) - 1
        self._want = None

    def add_pairs(self, hi, lo, cnt):
        self.pairs.append((hi, lo, cnt))
        self._want = None

    def reads_table(self, hb, ho):
        if self.lr:
            return self.oracle.count_lr(hb, ho)
        return self.oracle.count_kmers(hb, ho, self.k, self.canonical, method=1)

    def want(self):
        if self._want is None:
            if self.n_reads:
                t = self.reads_table(np.concatenate(self.b), np.concatenate(self.o).astype(np.uint64))
                his, los, cnts = [t.key_hi], [t.key_lo], [t.count]
            else:
                his, los, cnts = [], [], []
            for hi, lo, cnt in self.pairs:
                his.append(hi); los.append(lo); cnts.append(cnt)
            if his:
                hi, lo, cnt = slab_np.merge_sorted(his, los, cnts)
            else:
                hi, lo, cnt, _ = _empty(self.klen)
            self._want = self.kmc.Table(hi, lo, cnt, self.klen)
        return self._want


def _dev_reads(torch, hb, ho):
    """(bases, offsets) as device tensors (16-byte padded bases), ready on return."""
    d_b = torch.from_numpy(np.concatenate([hb, np.zeros(64, np.uint8)])).cuda()
    d_o = torch.from_numpy(np.asarray(ho, np.uint64).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return d_b, d_o


def _dev_pairs(torch, hi, lo, cnt):
    t = [torch.from_numpy(np.asarray(a, np.uint64).view(np.int64).copy()).cuda() for a in (hi, lo, cnt)]
    torch.cuda.synchronize()
    return t


def _write_fasta(path, hb, ho):
    with open(path, "wb") as f:
        for i in range(len(ho) - 1):
            f.write(b">r%d\n" % i)
            f.write(hb[int(ho[i]):int(ho[i + 1])].tobytes())
            f.write(b"\n")


class _Adder:
    """The four ways of adding to a ctx, each mirrored into the model.  Device buffers are kept alive until the next
    synchronising call (kmc.h: kmc_add_batch_device) -- here: until the adder is dropped."""

    def __init__(self, kmc, oracle, kc, model, tmp_path):
        self.kmc, self.oracle, self.kc, self.m, self.tmp = kmc, oracle, kc, model, tmp_path
        self.keep = []
        self.files = {}

    def add_batch(self, hb, ho):
        self.kc.add_batch(hb, ho)
        self.m.add_reads(hb, ho)

    def add_batch_device(self, hb, ho):
        d_b, d_o = _dev_reads(_torch(), hb, ho)
        self.keep.append((d_b, d_o))
        self.kc.add_batch_device(d_b.data_ptr(), d_o.data_ptr(), len(ho) - 1, int(ho[-1]), 0)
        self.m.add_reads(hb, ho)

    def count_file(self, hb, ho, tag):
        """kmc_count_file adds the file to the table and finalizes: its sizes are the model's."""
        if tag not in self.files:
            p = str(self.tmp / ("%s.fasta" % tag))
            _write_fasta(p, hb, ho)
            self.files[tag] = (p,) + tuple(self.oracle.parse_fasta(p))
        p, fb, fo = self.files[tag]
        nd, nt = self.kc.count_file(p)
        self.m.add_reads(fb, fo)
        w = self.m.want()
        assert (nd, nt) == (w.n_distinct, w.n_total), ("count_file", nd, nt, w.n_distinct, w.n_total)

    def merge_pairs(self, hi, lo, cnt):
        d_hi, d_lo, d_cnt = _dev_pairs(_torch(), hi, lo, cnt)
        self.keep.append((d_hi, d_lo, d_cnt))
        self.kc.merge_pairs_device(d_hi.data_ptr() if self.m.klen > 32 else 0, d_lo.data_ptr(), d_cnt.data_ptr(), len(lo))
        self.m.add_pairs(np.asarray(hi, np.uint64) if self.m.klen > 32 else np.zeros(len(lo), np.uint64),
                         np.asarray(lo, np.uint64), np.asarray(cnt, np.uint64))


def _check_export(kc, m, ctx=""):
    w = m.want()
    got = kc.export()
    assert got.equals(w), (ctx, got.n_distinct, w.n_distinct, got.n_total, w.n_total)
    st = kc.stats()
    assert st.n_kmers == w.n_total and st.n_reads == m.n_reads and st.n_planner_stale == 0, \
        (ctx, st.n_kmers, w.n_total, st.n_reads, m.n_reads, st.n_planner_stale)
    return got


def _check_hist(kc, w, n_bins=1001, lo=1, hi=0):
    h, mx = kc.histogram(n_bins, lo, hi, return_max=True)
    wh, wmx = _np_hist(w.count, n_bins, lo, hi)
    assert np.array_equal(h, wh) and mx == wmx, (n_bins, lo, hi, mx, wmx)


def _check_filtered(kc, w, lo, hi):
    m = _np_mask(w.count, lo, hi)
    f = kc.export_filtered(lo, hi)
    assert np.array_equal(f.key_lo, w.key_lo[m]) and np.array_equal(f.key_hi, w.key_hi[m]) and np.array_equal(f.count, w.count[m]), (lo, hi)


def _check_filter_device(kc, w, lo, hi):
    m = _np_mask(w.count, lo, hi)
    dhi, dlo, dcnt, nk, tot = kc.filter_device(lo, hi)
    assert nk == int(m.sum()) and tot == int(w.count[m].sum(dtype=np.uint64)), (lo, hi, nk, tot)
    if nk:
        assert np.array_equal(_dev_u64(dlo, nk), w.key_lo[m]) and np.array_equal(_dev_u64(dcnt, nk), w.count[m])
        if w.klen > 32:
            assert np.array_equal(_dev_u64(dhi, nk), w.key_hi[m])


def _check_export_device(kc, w):
    dhi, dlo, dcnt, n = kc.export_device()
    assert n == w.n_distinct, (n, w.n_distinct)
    if n:
        assert np.array_equal(_dev_u64(dlo, n), w.key_lo) and np.array_equal(_dev_u64(dcnt, n), w.count)
        if w.klen > 32:
            assert np.array_equal(_dev_u64(dhi, n), w.key_hi)
        else:
            assert dhi == 0


def _check_partition(kmc, kc, w, n_parts):
    pb, dhi, dlo, dcnt = kc.partition_device(n_parts)
    n = w.n_distinct
    assert pb[0] == 0 and pb[-1] == n and all(pb[i] <= pb[i + 1] for i in range(n_parts))
    lo, cnt = _dev_u64(dlo, n), _dev_u64(dcnt, n)
    hi = _dev_u64(dhi, n) if w.klen > 32 else np.zeros(n, np.uint64)
    for p in range(n_parts):
        for i in range(pb[p], pb[p + 1], max(1, (pb[p + 1] - pb[p]) // 64)):   # (a sample per part: ctypes calls)
            assert kmc.owner_of(int(hi[i]), int(lo[i]), n_parts) == p
    h2, l2, c2 = slab_np.merge_sorted([hi], [lo], [cnt])
    assert np.array_equal(h2, w.key_hi) and np.array_equal(l2, w.key_lo) and np.array_equal(c2, w.count)


def _reads(kmc, seed, pool, n_rec, first=0):
    return kmc.synth_reads_host(kmc.Synth(seed=seed, pool=pool), first, n_rec)


# ---- deterministic regressions ------------------------------------------------------------------------------------

ADDS = ["add_batch", "add_batch_device", "count_file", "merge_pairs"]


@pytest.mark.parametrize("k", [31, 63])
@pytest.mark.parametrize("synced", [False, True])
def test_add_behind_unobserved_async_finalize(kmc, oracle, tmp_path, k, synced):
    """A learned small-table source: add -> finalize_async -> [sync] -> add' -> export, add' each of the four ways of
    adding.  The queued finalize drained the table into the view (n_async_ok + 1 at the call that resolves it); add'
    has to put those counts back first: the export is the oracle's table of both additions (2x for repeated input)."""
    for pool in (10, 40):
        hb, ho = _reads(kmc, 70 + pool, pool, 6000)
        for how in ADDS:
            with kmc.KmerCounter(k=k) as kc:
                m = _Model(kmc, oracle, k, True)
                a = _Adder(kmc, oracle, kc, m, tmp_path)
                a.add_batch(hb, ho)
                _check_export(kc, m, "learn")                  # (learn the source: later batches go out in one launch)
                kc.reset(); m.reset()
                a.add_batch(hb, ho)
                ok0 = kc.stats().n_async_ok
                kc.finalize_async()
                if synced:
                    kc.sync()                                   # the kernel has certainly published
                w1 = m.reads_table(hb, ho)
                if how == "count_file":
                    a.count_file(hb, ho, "same")               # (the file holds the same reads)
                elif how == "merge_pairs":
                    a.merge_pairs(w1.key_hi, w1.key_lo, w1.count)
                else:
                    getattr(a, how)(hb, ho)
                d = kc.stats().n_async_ok - ok0                # (the call that resolved the queued finalize)
                t = _check_export(kc, m, (pool, how, synced))
                assert np.array_equal(t.key_lo, w1.key_lo) and np.array_equal(t.count, w1.count * 2), (pool, how)
                # the queued finalize drained the table (count_file finalizes once more itself)
                assert d in ((1, 2) if how == "count_file" else (1,)), (pool, how, synced, d)


def test_add_behind_async_finalize_that_gave_up(kmc, oracle, tmp_path):
    """finalize_async on a table the kernel refuses (far more than 131072 distinct keys, no sorted runs: ALGO_STREAM on
    all-distinct reads): nothing is drained, n_async_ok stays; each way of adding behind it and the export are exact."""
    hb, ho = _reads(kmc, 77, 0, 1500)
    assert oracle.count_kmers(hb, ho, 31, True, method=1).n_distinct > SMALL_MAX
    sb, so = _reads(kmc, 78, 10, 2000)
    for how in ADDS:
        with kmc.KmerCounter(k=31, algo=kmc.ALGO_STREAM) as kc:
            m = _Model(kmc, oracle, 31, True)
            a = _Adder(kmc, oracle, kc, m, tmp_path)
            a.add_batch(hb, ho)
            ok0 = kc.stats().n_async_ok
            kc.finalize_async()
            if how == "count_file":
                a.count_file(sb, so, "small")
            elif how == "merge_pairs":
                w1 = m.reads_table(sb, so)
                a.merge_pairs(w1.key_hi, w1.key_lo, w1.count)
                assert kc.stats().n_async_ok == ok0, how
            else:
                getattr(a, how)(sb, so)
                assert kc.stats().n_async_ok == ok0, how
            _check_export(kc, m, how)


@pytest.mark.parametrize("algo_name", ["walk", "auto"])
def test_reset_behind_async_finalize_then_recovery(kmc, oracle, algo_name):
    """add(lo) -> finalize_async -> reset -> add(hi) -> export, with the low/high pair of
    test_wrong_prediction_is_recovered_not_fatal: hi goes out in one launch planned on lo's history, overflows, and the
    recovery puts back the counters saved in front of it.  Those must be the EMPTY table's, not what the queued
    finalize published about lo after the reset.  Once and after several queued steps."""
    algo = {"walk": kmc.ALGO_WALK, "auto": kmc.ALGO_AUTO}[algo_name]
    k = 31
    lo_b, lo_o = _reads(kmc, 21, 10, 300_000)
    hi_b, hi_o = _reads(kmc, 22, 0, 12_000)
    want = oracle.count_kmers(hi_b, hi_o, k, True, method=1)
    want_lo = oracle.count_kmers(lo_b, lo_o, k, True, method=1)
    for steps in (1, 4):
        with kmc.KmerCounter(k=k, algo=algo) as kc:
            kc.add_batch(lo_b, lo_o)
            kc.finalize()
            ok0 = kc.stats().n_async_ok
            for _ in range(steps):
                kc.reset()
                kc.add_batch(lo_b, lo_o)
                kc.finalize_async()
            kc.reset()
            kc.add_batch(hi_b, hi_o)
            got = kc.export()
            st = kc.stats()
            assert got.equals(want), (algo_name, steps, got.n_distinct, want.n_distinct, got.n_total, want.n_total)
            assert st.n_kmers == want.n_total and st.n_reads == len(hi_o) - 1 and st.n_planner_stale == 0, \
                (algo_name, steps, st.n_kmers, want.n_total)
            kc.poll()
            assert kc.stats().n_async_ok - ok0 == steps, (algo_name, steps, "the queued finalizes did not all drain")
            kc.reset()
            kc.add_batch(lo_b, lo_o)
            assert kc.export().equals(want_lo)


@pytest.mark.parametrize("k", [31, 63])
def test_observers_straight_after_async_finalize(kmc, oracle, k):
    """Every look at the view with nothing but kmc_finalize_async in front of it: histogram, export_filtered,
    filter_device, export_device, partition_device, poll, forget_source -- each gives the oracle's result; a small
    table's queued finalize produced the view (n_async_ok + 1), a large one's gave up and the call finalized the
    ordinary way."""
    small = _reads(kmc, 90, 10, 5000)
    big = _reads(kmc, 91, 0, 1200)
    observers = ["histogram", "export_filtered", "filter_device", "export_device", "partition_device", "poll", "forget_source"]
    for src, (hb, ho) in (("small", small), ("big", big)):
        w = oracle.count_kmers(hb, ho, k, True, method=1)
        with kmc.KmerCounter(k=k, algo=kmc.ALGO_STREAM if src == "big" else kmc.ALGO_AUTO) as kc:
            for obs in observers:
                kc.reset()
                kc.add_batch(hb, ho)
                if src == "small":
                    kc.export()                                # (learned source, table size known: the queued kernel takes it)
                    kc.reset()
                    kc.add_batch(hb, ho)
                ok0 = kc.stats().n_async_ok
                kc.finalize_async()
                if obs == "histogram":
                    _check_hist(kc, w, 1001)
                    _check_hist(kc, w, 3, 2, 0)
                elif obs == "export_filtered":
                    _check_filtered(kc, w, 2, 0)
                elif obs == "filter_device":
                    _check_filter_device(kc, w, 2, 5)
                elif obs == "export_device":
                    _check_export_device(kc, w)
                elif obs == "partition_device":
                    _check_partition(kmc, kc, w, 4)
                elif obs == "poll":
                    kc.poll()
                else:
                    kc.forget_source(memo=True, history=False)
                d = kc.stats().n_async_ok - ok0
                assert d == (1 if src == "small" else 0), (src, obs, d)
                t = kc.export()
                assert t.equals(w), (src, obs)
                st = kc.stats()
                assert st.n_kmers == w.n_total and st.n_reads == len(ho) - 1 and st.n_planner_stale == 0, (src, obs)


def test_async_finalize_on_torch_stream(kmc, oracle):
    """The same orderings on a caller-provided torch stream (bench.py --gpus: ctxs on the training stream)."""
    torch = _torch()
    hb, ho = _reads(kmc, 95, 10, 5000)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        for k in (31, 63):
            w = oracle.count_kmers(hb, ho, k, True, method=1)
            with kmc.KmerCounter(k=k, stream=st.cuda_stream) as kc:
                kc.add_batch(hb, ho)
                kc.finalize()
                for rep in range(3):
                    kc.reset()
                    kc.add_batch(hb, ho)
                    ok0 = kc.stats().n_async_ok
                    kc.finalize_async()
                    kc.add_batch(hb, ho)                        # adding behind the queued finalize
                    assert kc.stats().n_async_ok - ok0 == 1
                    t = kc.export()
                    assert np.array_equal(t.key_lo, w.key_lo) and np.array_equal(t.count, w.count * 2), (k, rep)
                    kc.finalize_async()
                    kc.reset()                                  # resetting behind it
                    kc.add_batch(hb, ho)
                    kc.finalize_async()
                    _check_hist(kc, w, 1001)
                    assert kc.export().equals(w), (k, rep)


# ---- model-based random sequences ---------------------------------------------------------------------------------

TARGETS = ("add_batch", "add_batch_device", "count_file", "merge_pairs", "reset", "histogram")
MUTATORS = ("add_batch", "add_batch_device", "count_file", "merge_pairs", "reset", "forget_source")
OBSERVERS = ("export", "histogram", "export_filtered", "filter_device", "export_device", "poll", "sync", "stats")


def test_async_finalize_randomised_sequences(kmc, oracle, tmp_path):
    """A fixed-seed sibling of test_planner_randomised_batch_sequences: random sequences of every mutator (add_batch,
    add_batch_device, count_file, merge_pairs_device, reset, forget_source), both finalizes and every observer on one
    ctx, under all four algorithms, k in {21, 31, 47, 48, 63}, both strands and a few LR cases.  Small-table sources
    make the queued finalize succeed, all-distinct ones make it give up.  Every observation equals a host model of
    everything added since the last reset.  The test counts the transitions it exercised right behind a queued
    finalize that produced its view, and fails if one of finalize_async -> {add_batch, add_batch_device, count_file,
    merge_pairs, reset, histogram} never happened."""
    torch = _torch()
    rng = np.random.default_rng(int(os.environ.get("KMC_ASYNC_SEED", "20261016")))
    n_cases = int(os.environ.get("KMC_ASYNC_CASES", "28"))
    algos = [kmc.ALGO_AUTO, kmc.ALGO_WALK, kmc.ALGO_STREAM, kmc.ALGO_SORT]
    seen = {t: 0 for t in TARGETS}
    tried = {t: 0 for t in TARGETS}   # (the same transitions whatever the queued finalize's outcome)
    for case in range(n_cases):
        lr = case % 7 == 6
        k = 54 if lr else int(rng.choice([21, 31, 47, 48, 63]))
        algo = algos[case % 4]
        canonical = bool(rng.integers(0, 2))
        big_source = rng.random() < 0.3
        src_seed = int(rng.integers(1, 1 << 30))
        small_pool = 10       # (3-6 k distinct keys: the queued kernel takes the table even before it has seen one)
        with kmc.KmerCounter(k=k, canonical=canonical, algo=algo, mode=kmc.MODE_LR if lr else kmc.MODE_CONTIG) as kc:
            m = _Model(kmc, oracle, k, canonical, lr)
            a = _Adder(kmc, oracle, kc, m, tmp_path / ("c%d" % case))
            (tmp_path / ("c%d" % case)).mkdir()
            view = False          # a view (finalized or queued) of everything the model holds
            queued = None         # n_async_ok before the last finalize_async, while its outcome is unresolved
            behind_reset = None   # the same, for a finalize_async that a reset came behind
            label = None          # the call right behind that finalize_async

            def batch():
                pool = 0 if (big_source and rng.random() < 0.5) else small_pool
                n_rec = int(rng.integers(300, 1500 if pool == 0 else 3000))
                return pool, _reads(kmc, src_seed + pool, pool, n_rec, int(rng.integers(0, 2000)))

            def pairs():
                pb, po = _reads(kmc, src_seed + small_pool, small_pool, int(rng.integers(20, 200)), int(rng.integers(0, 2000)))
                t = m.reads_table(pb, po)
                cnt = rng.integers(1, 1000, size=t.n_distinct).astype(np.uint64)
                return t.key_hi, t.key_lo, cnt

            def resolved(what):
                """the call that looked at a queued finalize's outcome: n_async_ok tells whether it drained the table"""
                nonlocal queued, label
                if queued is None:
                    return
                d = kc.stats().n_async_ok - queued
                ok = d == 2 if what == "count_file" else d == 1     # (count_file finalizes once more itself)
                if label in tried:
                    tried[label] += 1
                assert d >= 0 and (d <= 2 if what == "count_file" else d <= 1), (case, what, d)
                if ok and label in seen:
                    seen[label] += 1
                queued = label = None

            # learn the source first (memo, launch history, the table's size): later queued finalizes take the table
            hb, ho = _reads(kmc, src_seed + small_pool, small_pool, 6000)
            a.add_batch(hb, ho)
            _check_export(kc, m, (case, "learn"))
            view = True
            n_ops = int(rng.integers(8, 16))
            prev = None
            for op_i in range(n_ops):
                if prev == "finalize_async" and rng.random() < 0.9:
                    op = str(rng.choice(TARGETS))
                elif prev == "reset_after_async":
                    op = str(rng.choice(["add_batch", "add_batch_device", "merge_pairs"]))
                elif prev in ("add_batch", "add_batch_device", "merge_pairs") and rng.random() < 0.7:
                    op = "finalize_async"                               # (queue one behind an addition: not a no-op)
                else:
                    op = str(rng.choice(MUTATORS + ("finalize", "finalize_async", "finalize_async") + OBSERVERS))
                if op in ("histogram", "export_filtered", "filter_device", "export_device") and not view:
                    op = "export"
                if prev == "finalize_async":
                    label = op
                ctx = (case, op_i, op, k, algo, canonical, lr)
                if op in ("add_batch", "add_batch_device", "count_file"):
                    pool, (hb, ho) = batch()
                    if op == "count_file":
                        a.count_file(hb, ho, "p%d" % pool)
                        view = True
                    else:
                        getattr(a, op)(hb, ho)
                        view = False
                    resolved(op)
                elif op == "merge_pairs":
                    a.merge_pairs(*pairs())
                    view = False
                    resolved(op)
                elif op == "reset":
                    kc.reset(); m.reset()
                    view = False
                    if queued is not None:
                        # the queued finalize's outcome is read at the next counter poll: after the next addition (the
                        # state its late publication used to spoil), a poll tells
                        behind_reset, queued, label = queued, None, None
                        op = "reset_after_async"
                elif op == "forget_source":
                    kc.forget_source(memo=bool(rng.integers(0, 2)), history=bool(rng.integers(0, 2)))
                    resolved(op)
                elif op == "finalize":
                    w = m.want()
                    assert kc.finalize() == (w.n_distinct, w.n_total), ctx
                    view = True
                    resolved(op)
                elif op == "finalize_async":
                    if queued is None:
                        queued = kc.stats().n_async_ok
                    kc.finalize_async()
                    view = True
                elif op == "export":
                    _check_export(kc, m, ctx)
                    view = True
                    resolved(op)
                elif op == "histogram":
                    _check_hist(kc, m.want(), int(rng.choice([2, 17, 1001])), int(rng.integers(1, 3)), 0)
                    resolved(op)
                elif op == "export_filtered":
                    _check_filtered(kc, m.want(), int(rng.integers(1, 4)), int(rng.choice([0, 3, 50])))
                    resolved(op)
                elif op == "filter_device":
                    lo = int(rng.integers(1, 4))
                    _check_filter_device(kc, m.want(), lo, int(rng.choice([0, lo, 50])))
                    resolved(op)
                elif op == "export_device":
                    _check_export_device(kc, m.want())
                    resolved(op)
                elif op == "poll":
                    kc.poll()
                    resolved(op)
                elif op == "sync":
                    kc.sync()
                elif op == "stats":
                    st = kc.stats()
                    assert st.n_reads == m.n_reads and st.n_planner_stale == 0, ctx
                if prev == "reset_after_async":
                    # the finalize queued in front of the reset: its outcome, now that an addition ran behind the reset
                    kc.poll()
                    d = kc.stats().n_async_ok - behind_reset
                    assert d in (0, 1), (ctx, d)
                    tried["reset"] += 1
                    if d == 1:
                        seen["reset"] += 1
                prev = op
            _check_export(kc, m, (case, "end"))
            assert kc.stats().n_planner_stale == 0
    missing = [t for t, n in seen.items() if n == 0]
    if missing:
        pytest.fail("finalize_async -> %s never ran behind a queued finalize that drained the table (drained: %s, all: %s)"
                    % (missing, seen, tried))
