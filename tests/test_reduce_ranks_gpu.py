"""The multi-GPU count-table reduce (k-mer-count_amd/distributed.py) with REAL contexts at world 1, 2 and 3: fresh child
processes (spawn start method) share GPU 0 over a gloo group -- RCCL refuses two ranks on one device -- so the owner
filter of kmc_merge_slabs_kernel, the one-rank-oversize route through the all-to-all, kmc_partition_device with more
than one part, the device-tensor branches of all_to_all_v / _all_gather_slabs, the deferred path
reduce_tables(finalize=False) and the global_* calls run on kernels, streams and pinned counters instead of the numpy
stand-in of tests/slab_np.py.  One spawn per world size runs all of that world's cases; every rank asserts its own
partition against the oracle's whole table, the parent asserts what needs all ranks (disjoint parts that add up).

Further down, in this process: kmc_partition_device checked entry by entry at 1..4096 parts.

Not covered here (nor anywhere): RCCL with more than one rank, peer copies between distinct devices."""
import contextlib
import datetime
import importlib
import json
import os
import socket
import sys
import time

import numpy as np
import pytest

import partition_np as P
from conftest import ROOT, SAMPLE

pytestmark = pytest.mark.gpu

# (k, slab_entries, ranks whose shard table does not fit the slab) per world size; the shards are the uneven record cuts
# of tests/test_distributed_cpu.py:_worker_reduce (2 records | the rest, 2 | 3 | the rest)
CASES = {
    2: [(31, 8192, 0), (63, 8192, 0), (31, 2000, 1), (63, 16, 2),
        (1, 1, 2)],        # two canonical 1-mers, both owned by rank 0: an all-to-all with empty parts and zero-size sends
    3: [(63, 3000, 1), (31, 600, 2), (63, 8, 3),
        (1, 8192, 0)],     # rank 2 owns nothing
}
MODES = ("own", "side")    # both ctxs on their own streams / both on one torch side stream (as bench.py sets them up)
STEPS = 4                  # steps of a deferred sequence
# record windows [first, first + n) of the sample per step: all different, so that a view left over from an earlier
# step is a visible error
STEADY = [(0, 12), (40, 20), (90, 9), (150, 30)]
# the same with ONE step (the third) far larger than the others: with the slab sized between them exactly one rank's
# table of exactly that step is oversize
ONE_BIG = [(0, 8), (20, 7), (40, 80), (130, 9)]
BIG_STEP = 2
COMPARE_RANGES = ((1, 0, 1, 0), (3, 0, 1, 40))
HISTOS = ((10001, 1, 0), (40, 2, 100))

# Wall time of one spawn (start of fresh processes that import torch, open the GPU and load the library, all of a
# world's sections, join), measured on an MI355X machine: 2.2 s (world 1), 2.5-2.9 s (world 2), 2.7-3.1 s (world 3) -- of
# which the sections take 0.15-0.3 s --, and 8.8 s for the first spawn on a machine that had not run anything yet.  The
# deadline is about five times the slowest.  At the deadline the children are terminated and the test fails.
SPAWN_SECONDS_MEASURED = {1: 2.2, 2: 8.8, 3: 3.1}
SPAWN_DEADLINE_S = 45.0


def _bounds(n_reads, world):
    cut = 2
    if world == 1:
        return [0, n_reads]
    if world == 2:
        return [0, cut, n_reads]
    return [0, cut, cut + 3] + [n_reads] * (world - 2)


def _queries(whole):
    """present keys (with repeats), neighbours of present keys, and three small constants"""
    rng = np.random.default_rng(7)
    pick = rng.integers(0, whole.n_distinct, 3000)
    hi = np.concatenate([whole.key_hi[pick], whole.key_hi[:50], np.zeros(3, np.uint64)])
    lo = np.concatenate([whole.key_lo[pick], whole.key_lo[:50] ^ np.uint64(1), np.array([0, 1, 2], np.uint64)])
    return hi, lo


def _np_hist(counts, n_bins, lo=1, hi=0):
    c = counts.astype(np.uint64)
    keep = (c >= np.uint64(lo)) & ((c <= np.uint64(hi)) if hi else True)
    return np.bincount(np.minimum(c[keep], np.uint64(n_bins - 1)).astype(np.int64), minlength=n_bins).astype(np.uint64), \
        (int(c[keep].max()) if keep.any() else 0)


# ---- what runs in the children --------------------------------------------------------------------------------------

class _Rank:
    """One rank's side of a spawn: the sample, oracle tables of record ranges, and a pair of ctxs per (k, mode)."""

    def __init__(self, rank, world, outdir):
        import torch
        import oracle_py
        self.torch = torch
        self.rank, self.world, self.outdir = rank, world, outdir
        self.kmc = importlib.import_module("k-mer-count_amd")
        self.kd = importlib.import_module("k-mer-count_amd.distributed")
        self.oracle = oracle_py
        self.kmc.lib()
        self.bases, self.offs = oracle_py.parse_fasta(SAMPLE)
        self.n_reads = len(self.offs) - 1
        self.side = torch.cuda.Stream()
        self._tabs = {}
        self._ctxs = {}
        self.done = []
        self.seconds = {}

    def reads(self, r0, r1):
        return self.bases[int(self.offs[r0]):int(self.offs[r1])], self.offs[r0:r1 + 1] - self.offs[r0]

    def table(self, k, r0, r1):
        if (k, r0, r1) not in self._tabs:
            self._tabs[(k, r0, r1)] = self.oracle.count_kmers(*self.reads(r0, r1), k, True)
        return self._tabs[(k, r0, r1)]

    def shard(self, r0, r1, rank=None):
        """record range of `rank` (default: this one) of the window [r0, r1)"""
        b = _bounds(r1 - r0, self.world)
        r = self.rank if rank is None else rank
        return r0 + b[r], r0 + b[r + 1]

    def on(self, mode):
        return self.torch.cuda.stream(self.side) if mode == "side" else contextlib.nullcontext()

    def ctxs(self, k, mode, n=2):
        key = (k, mode)
        have = self._ctxs.setdefault(key, [])
        while len(have) < n:
            have.append(self.kmc.KmerCounter(k=k, stream=self.side.cuda_stream if mode == "side" else None))
        return have[:n]

    def close(self):
        for have in self._ctxs.values():
            for kc in have:
                kc.close()

    def check_owned(self, owner, whole, what):
        """owner.export() is this rank's part of `whole`: key for key, in order, count for count"""
        hi, lo, cnt = P.owned(whole, self.world, self.rank)
        t = owner.export()
        assert t.n_distinct == len(lo), (what, self.rank, t.n_distinct, len(lo))
        assert np.array_equal(t.key_hi, hi) and np.array_equal(t.key_lo, lo), (what, self.rank, "keys")
        # (a slab or a part merged twice shows here: the sum is too large)
        assert np.array_equal(t.count, cnt), (what, self.rank, "counts differ: sum", int(t.count.sum()), "want", int(cnt.sum()))
        return t

    def step(self, local, owner, k, window, slab_entries, finalize):
        r0, r1 = window[0], window[0] + window[1]
        local.reset()
        local.add_batch(*self.reads(*self.shard(r0, r1)))
        owner.reset()
        return self.kd.reduce_tables(local, owner, slab_entries=slab_entries, finalize=finalize)

    def timed(self, name, fn):
        t0 = time.perf_counter()
        fn()
        self.seconds[name] = round(time.perf_counter() - t0, 3)
        self.done.append(name)


def _section_reduce(R):
    """A: reduce_tables(finalize=True), every case of this world, both stream set-ups; then the global_* calls"""
    kd, world, rank = R.kd, R.world, R.rank
    for mode in MODES:
        for k, E, n_over in CASES[world]:
            what = ("reduce", world, k, E, mode)
            whole = R.table(k, 0, R.n_reads)
            sizes = [R.table(k, *R.shard(0, R.n_reads, r)).n_distinct for r in range(world)]
            assert sum(1 for s in sizes if s > E) == n_over, (what, sizes)     # the case is what its row says
            local, owner = R.ctxs(k, mode)
            with R.on(mode):
                sent, got = R.step(local, owner, k, (0, R.n_reads), E, True)
                mine = kd.owner_np(whole.key_hi, whole.key_lo, world) == rank
                t = R.check_owned(owner, whole, what)
                assert sent == sizes[rank], (what, rank, sent, sizes)
                assert got == int(mine.sum()), (what, rank, got, int(mine.sum()))
                assert owner.stats().n_slabs_skipped == n_over, (what, rank, owner.stats().n_slabs_skipped)
                np.savez(os.path.join(R.outdir, "A_%s_%d_%d_r%d.npz" % (mode, k, E, rank)), hi=t.key_hi, lo=t.key_lo, cnt=t.count)
                # the finalized owners answer for the whole table
                qhi, qlo = _queries(whole)
                table = {(int(h), int(l)): int(c) for h, l, c in zip(whole.key_hi, whole.key_lo, whole.count)}
                want = np.array([table.get((int(h), int(l)), 0) for h, l in zip(qhi, qlo)], np.uint64)
                assert want[:3000].all()
                assert np.array_equal(kd.global_query(owner, qhi if k > 31 else None, qlo), want), what
                for n_bins, lo, hi in HISTOS:
                    h, mx = kd.global_histogram(owner, n_bins, lo, hi)
                    wh, wmx = _np_hist(whole.count, n_bins, lo, hi)
                    assert np.array_equal(h, wh) and mx == wmx, (what, n_bins, lo, hi)


def _section_compare(R):
    """global_compare of two samples, each reduced into its own owner ctx"""
    import setops_np as M
    n = R.n_reads
    for k in (31, 63):
        local, oa, ob = R.ctxs(k, "side", 3)
        spans = ((0, 2 * n // 3), (n // 3, n))
        with R.on("side"):
            for owner, (r0, r1) in zip((oa, ob), spans):
                R.step(local, owner, k, (r0, r1 - r0), 8192, True)
            a, b = (R.table(k, r0, r1) for r0, r1 in spans)
            R.check_owned(oa, a, ("compare a", k))
            R.check_owned(ob, b, ("compare b", k))
            for r in COMPARE_RANGES:
                want = M.summary(M.of(a), M.of(b), *r)
                c = R.kd.global_compare(oa, ob, *r)
                assert [int(w) for w in c.words()] == want, (k, r, c.words(), want)
                assert want[2] > 0


def _window_tables(R, k, windows):
    return [R.table(k, w[0], w[0] + w[1]) for w in windows]


def _section_steady(R):
    """B.1: S deferred steps, every one on a different record range; then one look"""
    for k in (31, 63):
        local, owner = R.ctxs(k, "side")
        with R.on("side"):
            owner.finalize()
            st0 = owner.stats()
            for w in STEADY:
                assert R.step(local, owner, k, w, 8192, False) == (None, None)
            owner.finalize()
            st = owner.stats()
            assert st.n_async_ok - st0.n_async_ok == STEPS, (k, R.rank, st.n_async_ok - st0.n_async_ok)
            assert st.n_async_slabs_skipped == st0.n_async_slabs_skipped, (k, R.rank)
            R.check_owned(owner, _window_tables(R, k, STEADY)[-1], ("steady", k))


def _section_one_big(R):
    """B.2: one rank's table of one middle step does not fit its slab; what the counters say, then the recovery"""
    world = R.world
    for k in (31, 63):
        sizes = {(s, r): R.table(k, *R.shard(w[0], w[0] + w[1], r)).n_distinct for s, w in enumerate(ONE_BIG) for r in range(world)}
        target = (BIG_STEP, world - 1)
        E = max(v for sr, v in sizes.items() if sr != target)
        assert sizes[target] > E, (k, world, sizes)      # exactly one (step, rank) is oversize
        local, owner = R.ctxs(k, "side")
        with R.on("side"):
            owner.finalize()
            st0 = owner.stats()
            for w in ONE_BIG:
                assert R.step(local, owner, k, w, E, False) == (None, None)
            owner.finalize()
            st = owner.stats()
            # include/kmc.h: one per finalize that produced its view (every step did: the slabs that travelled inline,
            # possibly none), and the oversize slabs those finalizes saw (one, in the big step, seen by EVERY rank)
            assert st.n_async_ok - st0.n_async_ok == STEPS, (k, R.rank, st.n_async_ok - st0.n_async_ok)
            assert st.n_async_slabs_skipped - st0.n_async_slabs_skipped == 1, (k, R.rank, st.n_async_slabs_skipped - st0.n_async_slabs_skipped)
            tabs = _window_tables(R, k, ONE_BIG)
            R.check_owned(owner, tabs[-1], ("one big: last step", k))
            # the documented recovery: owner.reset(), the step again with finalize=True -- the exact partition, nothing doubled
            sent, got = R.step(local, owner, k, ONE_BIG[BIG_STEP], E, True)
            t = R.check_owned(owner, tabs[BIG_STEP], ("one big: redone step", k))
            assert sent == sizes[(BIG_STEP, R.rank)] and got == t.n_distinct
            assert int(t.count.sum()) == int(P.owned(tabs[BIG_STEP], world, R.rank)[2].sum())
            assert owner.stats().n_slabs_skipped == 1


def _section_empty_owner(R):
    """B.3: k = 1 -- two canonical keys, none of them owned by the last rank of 2 or of 3.  A step in which nothing was
    oversize counts as delivered on EVERY rank, also on one whose partition is empty."""
    k = 1
    whole_last = _window_tables(R, k, STEADY)[-1]
    mine = R.kd.owner_np(whole_last.key_hi, whole_last.key_lo, R.world) == R.rank
    if R.world > 1:
        assert (int(mine.sum()) == 0) == (R.rank == R.world - 1), (R.world, R.rank, int(mine.sum()))   # the last rank owns nothing
    local, owner = R.ctxs(k, "side")
    with R.on("side"):
        owner.finalize()
        st0 = owner.stats()
        for w in STEADY:
            assert R.step(local, owner, k, w, 8192, False) == (None, None)
        nd, nt = owner.finalize()
        st = owner.stats()
        assert st.n_async_ok - st0.n_async_ok == STEPS, ("empty owner", R.world, R.rank, st.n_async_ok - st0.n_async_ok)
        assert st.n_async_slabs_skipped == st0.n_async_slabs_skipped
        assert nd == int(mine.sum()) and nt == int(whole_last.count[mine].sum())
        R.check_owned(owner, whole_last, ("empty owner", k))
        # the empty view is a view: the calls that read it answer, and adding behind it works
        if not mine.any():
            pb, _, _, _ = owner.partition_device(3)
            assert pb == [0, 0, 0, 0]
            assert owner.export_device()[3] == 0
            assert not owner.histogram(5).any()
        sent, got = R.step(local, owner, k, STEADY[0], 8192, True)
        R.check_owned(owner, _window_tables(R, k, STEADY)[0], ("empty owner: a synchronous step behind", k))


def _section_precondition(R):
    """B.4: finalize=False with a ctx that is not on torch's current stream: ValueError before anything is queued"""
    k = 31
    pairs = [R.ctxs(k, "own"), R.ctxs(k, "side")]     # (the side-stream pair called OUTSIDE `with torch.cuda.stream(side)`)
    for local, owner in pairs:
        local.reset()
        local.add_batch(*R.reads(*R.shard(0, R.n_reads)))
        owner.reset()
        owner.finalize()
        ok0 = owner.stats().n_async_ok
        with pytest.raises(ValueError):
            R.kd.reduce_tables(local, owner, finalize=False)
        assert owner.stats().n_async_ok == ok0
        assert owner.export().n_distinct == 0
        assert owner.stats().n_slabs_skipped == 0


SECTIONS = {
    "reduce": _section_reduce,
    "compare": _section_compare,
    "steady": _section_steady,
    "one_big": _section_one_big,
    "empty_owner": _section_empty_owner,
    "precondition": _section_precondition,
}
SECTIONS_OF = {1: ("steady", "one_big", "empty_owner", "precondition"),
               2: ("reduce", "compare", "steady", "one_big", "empty_owner", "precondition"),
               3: ("reduce", "compare", "steady", "one_big", "empty_owner", "precondition")}


def _child(rank, world, port, outdir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    try:
        R = _Rank(rank, world, outdir)
        for name in SECTIONS_OF[world]:
            R.timed(name, lambda: SECTIONS[name](R))
            torch.cuda.synchronize()
        R.close()
        with open(os.path.join(outdir, "done_r%d.json" % rank), "w") as f:
            json.dump({"done": R.done, "seconds": R.seconds}, f)
        dist.barrier()
    finally:
        dist.destroy_process_group()


# ---- the parent -----------------------------------------------------------------------------------------------------

def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _spawn_world(world, outdir):
    """One spawn: `world` fresh children, all of that world's sections, joined against the deadline.  A child that
    exits non-zero raises here (torch terminates its partners); nothing is retried."""
    import torch.multiprocessing as mp
    t0 = time.perf_counter()
    ctx = mp.spawn(_child, args=(world, _free_port(), str(outdir)), nprocs=world, join=False)
    try:
        while not ctx.join(timeout=max(0.1, min(5.0, SPAWN_DEADLINE_S - (time.perf_counter() - t0)))):
            if time.perf_counter() - t0 > SPAWN_DEADLINE_S:
                pytest.fail("world %d: the children did not finish within %.0f s" % (world, SPAWN_DEADLINE_S))
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.terminate()
        for p in ctx.processes:
            p.join(10)
    wall = time.perf_counter() - t0
    done = [json.load(open(os.path.join(outdir, "done_r%d.json" % r))) for r in range(world)]
    print("world %d spawn: %.1f s wall; per section (rank 0): %s" % (world, wall, done[0]["seconds"]))
    return {"dir": str(outdir), "wall": wall, "done": done}


@pytest.fixture(scope="module")
def spawn1(kmc, oracle, tmp_path_factory):
    return _spawn_world(1, tmp_path_factory.mktemp("ranks1"))


@pytest.fixture(scope="module")
def spawn2(kmc, oracle, tmp_path_factory):
    return _spawn_world(2, tmp_path_factory.mktemp("ranks2"))


@pytest.fixture(scope="module")
def spawn3(kmc, oracle, tmp_path_factory):
    return _spawn_world(3, tmp_path_factory.mktemp("ranks3"))


def _check_parts(oracle, run, world, k, E, mode):
    parts = [np.load(os.path.join(run["dir"], "A_%s_%d_%d_r%d.npz" % (mode, k, E, r))) for r in range(world)]
    bases, offs = oracle.parse_fasta(SAMPLE)
    whole = oracle.count_kmers(bases, offs, k, True)
    # (every rank has already compared its part with whole[owner == rank], entry by entry)
    assert sum(len(p["lo"]) for p in parts) == whole.n_distinct
    keys = np.stack([np.concatenate([p["hi"] for p in parts]), np.concatenate([p["lo"] for p in parts])], axis=1)
    assert np.unique(keys, axis=0).shape[0] == keys.shape[0], "a key is owned twice"
    assert sum(int(p["cnt"].sum()) for p in parts) == whole.n_total


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k,slab_entries,n_over", CASES[2])
def test_world2_reduce_tables_real_contexts(oracle, spawn2, k, slab_entries, n_over, mode):
    _check_parts(oracle, spawn2, 2, k, slab_entries, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k,slab_entries,n_over", CASES[3])
def test_world3_reduce_tables_real_contexts(oracle, spawn3, k, slab_entries, n_over, mode):
    _check_parts(oracle, spawn3, 3, k, slab_entries, mode)


@pytest.mark.parametrize("world", [1, 2, 3])
def test_deferred_reduce_and_global_calls(request, world):
    """reduce_tables(finalize=False) -- steady state, a step that does not fit and its recovery, an owner whose partition
    is empty, the stream precondition -- and (world > 1) global_query / global_histogram / global_compare: every rank ran
    every section to its end (the assertions are in the sections, above)."""
    run = request.getfixturevalue("spawn%d" % world)
    for r in range(world):
        assert tuple(run["done"][r]["done"]) == SECTIONS_OF[world], (world, r, run["done"][r])


# ---- kmc_partition_device, every entry ------------------------------------------------------------------------------

N_PARTS = (1, 2, 3, 5, 8, 63, 64, 65, 257, 4096)   # 65 and more: more distinct owners in a wave than one round each serves


def _dev_u64(ptr, n):
    import torch
    kd = importlib.import_module("k-mer-count_amd.distributed")
    return kd.device_view(ptr, n, torch.device("cuda", 0)).cpu().numpy().view(np.uint64).copy()


def _partition_host(kc, n_parts, two_words):
    pb, dhi, dlo, dcnt = kc.partition_device(n_parts)
    n = pb[-1]
    assert not (two_words and n) or dhi
    hi = _dev_u64(dhi, n) if two_words else np.zeros(n, np.uint64)
    return pb, hi, _dev_u64(dlo, n), _dev_u64(dcnt, n)


def _check_all_parts(kc, w, two_words):
    for n_parts in N_PARTS:
        pb, hi, lo, cnt = _partition_host(kc, n_parts, two_words)
        P.check_partition(pb, hi, lo, cnt, w.key_hi, w.key_lo, w.count, n_parts)
        if n_parts == 4096 and 0 < w.n_distinct <= 6140:
            assert (np.diff(pb) == 0).any()          # parts are empty


@pytest.mark.parametrize("k", [31, 63])
def test_partition_every_entry_sample(kmc, oracle, k):
    bases, offs = oracle.parse_fasta(SAMPLE)
    w = oracle.count_kmers(bases, offs, k, True)
    with kmc.KmerCounter(k=k) as kc:
        kc.add_batch(bases, offs)
        kc.finalize()
        _check_all_parts(kc, w, k > 31)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 6140, 300_007])
@pytest.mark.parametrize("k", [31, 63])
def test_partition_every_entry_random_pairs(kmc, k, n):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(1000 * k + n % 997)
    lo = rng.integers(0, 2**62, n, dtype=np.uint64)
    hi = rng.integers(1, 2**60, n, dtype=np.uint64) if k > 31 else np.zeros(n, np.uint64)
    if k > 31:
        hi[: n // 2] = hi[0]
    cnt = rng.integers(1, 1000, n, dtype=np.uint64)
    assert np.unique(np.stack([hi, lo], axis=1), axis=0).shape[0] == n
    d = [torch.from_numpy(a.astype(np.int64)).cuda() for a in (hi, lo, cnt)]
    torch.cuda.synchronize()
    order = np.lexsort((lo, hi))
    w = kmc.Table(hi[order], lo[order], cnt[order], k)
    with kmc.KmerCounter(k=k) as kc:
        kc.merge_pairs_device(d[0].data_ptr() if k > 31 else 0, d[1].data_ptr(), d[2].data_ptr(), n)
        assert kc.finalize() == (n, int(cnt.sum()))
        _check_all_parts(kc, w, k > 31)


@pytest.mark.parametrize("k", [31, 63])
def test_partition_of_an_empty_view(kmc, k):
    with kmc.KmerCounter(k=k) as kc:
        assert kc.finalize() == (0, 0)
        for n_parts in N_PARTS:
            pb, _, _, _ = kc.partition_device(n_parts)
            assert pb == [0] * (n_parts + 1)


def test_partition_argument_errors_leave_results_alone(kmc, oracle):
    bases, offs = oracle.parse_fasta(SAMPLE)
    k = 63
    w = oracle.count_kmers(bases, offs, k, True)
    with kmc.KmerCounter(k=k) as kc:
        kc.add_batch(bases, offs)
        kc.finalize()
        pb, dhi, dlo, dcnt = kc.partition_device(5)
        before = (_dev_u64(dhi, pb[-1]), _dev_u64(dlo, pb[-1]), _dev_u64(dcnt, pb[-1]))
        for bad in (4097, 0):
            with pytest.raises(kmc.KmcError) as e:
                kc.partition_device(bad)
            assert e.value.status == kmc.ERR_ARG, bad
            # the earlier partition result, at the addresses it was handed out at, and the view
            after = (_dev_u64(dhi, pb[-1]), _dev_u64(dlo, pb[-1]), _dev_u64(dcnt, pb[-1]))
            assert all(np.array_equal(a, b) for a, b in zip(before, after)), bad
            P.check_partition(pb, *after, w.key_hi, w.key_lo, w.count, 5)
            vhi, vlo, vcnt, vn = kc.export_device()
            assert vn == w.n_distinct
            assert np.array_equal(_dev_u64(vhi, vn), w.key_hi) and np.array_equal(_dev_u64(vlo, vn), w.key_lo) and np.array_equal(_dev_u64(vcnt, vn), w.count)
        assert kc.export().equals(w)
