"""The walk path's rank plan (kmc_walk_plan.hip.h): a repeat batch is finalized by one small launch between the walk
kernel and its tail.  Every result is compared with the CPU oracle through Table.equals and the (nd, nt) of finalize
with the oracle's; kmc_stats.walk_plan_finalizes / walk_plan_builds prove which path delivered.

The plan launch finalizes only if the host has queued the finalize by the time the launch runs.  A 1,500-read walk
kernel is over in tens of microseconds, about what the host needs between the two calls, so the contexts here run on a
torch stream and every add is preceded by a fill of a large buffer on that stream (_Rig.hold): the GPU is a few hundred
microseconds behind the host, as it is behind every real batch, and which path delivers is decided by the library's
rules alone.  Where a test leaves the race open (a ctx on its own stream, a one-read batch) only exactness is asserted."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)
PLAN_MAX = 4096   # KMC_WALK_PLAN_MAX
N_READS = 1500    # 24 tiles, two workgroups


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "the gpu tests need a GPU"
    return t


class _Rig:
    """A torch stream for the contexts and the buffer whose fill holds that stream back."""

    def __init__(self, torch):
        self.torch = torch
        self.stream = torch.cuda.Stream()
        self.buf = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def hold(self, stream=None):
        with self.torch.cuda.stream(stream or self.stream):
            self.buf.zero_()

    def ctx(self, kmc, k, canonical=True, stream=None):
        return kmc.KmerCounter(k=k, canonical=canonical, algo=kmc.ALGO_WALK, stream=(stream or self.stream).cuda_stream)


@pytest.fixture(scope="module")
def rig(torch):
    return _Rig(torch)


def _lines(rng, n_lines, L):
    return ACGT[rng.integers(0, 4, (n_lines, L))]


def _batch(rng, lines, which, n_reads=N_READS):
    """n_reads reads, each one of lines[which] (every one of them occurs), all of one length."""
    which = np.asarray(which)
    pick = which[rng.integers(0, len(which), n_reads)]
    pick[:len(which)] = which
    bases = lines[pick].reshape(-1).copy()
    offs = np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(lines.shape[1])
    return bases, offs


class _Dev:
    """A batch on the device (padded: the 16-byte piece that holds the last base is readable) and its oracle table."""

    def __init__(self, torch, oracle, bases, offs, k, canonical):
        pad = np.full(len(bases) + 16, ord("N"), np.uint8)
        pad[:len(bases)] = bases
        self.bases, self.offs = bases, offs
        self.db, self.do = torch.from_numpy(pad).cuda(), torch.from_numpy(offs.astype(np.int64)).cuda()
        self.n_reads, self.n_bases = len(offs) - 1, len(bases)
        self.mrl = int(np.diff(offs.astype(np.int64)).max()) if self.n_reads else 0
        self.want = oracle.count_kmers(bases, offs, k, canonical)

    def add(self, kc):
        kc.add_batch_device(self.db.data_ptr(), self.do.data_ptr(), self.n_reads, self.n_bases, self.mrl)


def _concat(oracle, devs, k, canonical):
    bases = np.concatenate([d.bases for d in devs])
    lens = np.concatenate([np.diff(d.offs.astype(np.int64)) for d in devs])
    offs = np.zeros(len(lens) + 1, np.uint64)
    offs[1:] = np.cumsum(lens)
    return oracle.count_kmers(bases, offs, k, canonical)


def _counters(kc):
    st = kc.stats()
    return st.walk_plan_finalizes, st.walk_plan_builds


def _cycle(rig, kc, dev, want=None, tag=None, stream=None):
    """reset -> add_batch_device -> finalize, exact.  Returns (plan finalizes, plan builds, launches_last) it added / saw."""
    want = dev.want if want is None else want
    f0, b0 = _counters(kc)
    kc.reset()
    rig.hold(stream)
    dev.add(kc)
    nd, nt = kc.finalize()
    got = kc.export()
    kc.poll()
    st = kc.stats()
    print("cycle", tag, "nd", nd, "nt", nt, "plan finalizes +", st.walk_plan_finalizes - f0, "builds +", st.walk_plan_builds - b0, "launches_last", st.launches_last)
    assert (nd, nt) == (want.n_distinct, want.n_total), (tag, nd, nt, want.n_distinct, want.n_total)
    assert got.equals(want), tag
    return st.walk_plan_finalizes - f0, st.walk_plan_builds - b0, st.launches_last


def _planned(rig, kmc, kc, dev, tag):
    """Two cycles: the first builds the plan, the second is delivered by it."""
    assert _cycle(rig, kc, dev, tag=(tag, "learn"))[:2] == (0, 1)
    assert _cycle(rig, kc, dev, tag=(tag, "plan"))[:2] == (1, 0)


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [5, 31, 63])
@pytest.mark.parametrize("L", [64, 400])
def test_repeat_cycles(kmc, oracle, torch, rig, L, k, canonical):
    """Eight cycles of one pool batch on one ctx.  The cycle the design fixes on is the SECOND: the plan is built behind the
    first finalize whose table was one walk launch on an empty table -- the first cycle's (cold memo: every k-mer goes
    through the table, and workgroup 0, whose memo becomes the snapshot, has walked every pool line) -- and the second
    cycle runs from that snapshot, leaves the table empty and is gathered from the plan.  From then on the finalize
    counter grows by one per cycle and nothing is built.  k = 5: most items are SKIP or share a row.
    L = 400 at k = 31 has 12 * 370 = 4,440 distinct k-mers, more than KMC_WALK_PLAN_MAX: by the same rule no plan may
    be built and no cycle delivered by one (the expectation follows the oracle's row count, not the case's name)."""
    rng = np.random.default_rng(5000 + 100 * L + 2 * k + int(canonical))
    dev = _Dev(torch, oracle, *_batch(rng, _lines(rng, 12, L), np.arange(12)), k, canonical)
    fits = 1 <= dev.want.n_distinct <= PLAN_MAX
    assert fits or (L, k) == (400, 31)
    launches = set()
    with rig.ctx(kmc, k, canonical) as kc:
        for cyc in range(1, 9):
            fin, built, nl = _cycle(rig, kc, dev, tag=(L, k, canonical, cyc))
            launches.add(nl)
            assert built == (1 if fits and cyc == 1 else 0), (cyc, built)
            assert fin == (1 if fits and cyc >= 2 else 0), (cyc, fin)
    assert launches == {1}, launches   # (the plan launch is not a count launch)


def test_rows_that_vanish_and_lines_never_seen(kmc, oracle, torch, rig):
    """A batch of a strict subset of the pool lines behind the plan: rows with a zero count are dropped, nd is smaller.
    Then two lines the memo has never seen: the first cycle meets them in the table (an ordinary finalize), the next
    finds counters on items without a row (stale: an ordinary finalize and a rebuild), then the plan delivers again."""
    k, L = 31, 64
    rng = np.random.default_rng(77)
    lines = _lines(rng, 14, L)
    full = _Dev(torch, oracle, *_batch(rng, lines, np.arange(12)), k, True)
    sub = _Dev(torch, oracle, *_batch(rng, lines, np.arange(6)), k, True)
    more = _Dev(torch, oracle, *_batch(rng, lines, np.arange(14)), k, True)
    assert sub.want.n_distinct < full.want.n_distinct < more.want.n_distinct <= PLAN_MAX
    with rig.ctx(kmc, k) as kc:
        _planned(rig, kmc, kc, full, "full")
        assert _cycle(rig, kc, sub, tag="subset")[:2] == (1, 0)
        assert _cycle(rig, kc, full, tag="full again")[:2] == (1, 0)
        seen = [_cycle(rig, kc, more, tag=("more", i))[:2] for i in range(4)]
        assert seen[0] == (0, 0), seen                  # new entries: through the table
        assert sum(b for _, b in seen) == 1, seen       # one rebuild ...
        assert seen[-1] == (1, 0), seen                 # ... and the plan delivers again
        assert _cycle(rig, kc, sub, tag="subset behind the rebuild")[:2] == (1, 0)


def test_refusals(kmc, oracle, torch, rig, monkeypatch):
    """What the plan launch must leave to the ordinary path, each exact, the finalize counter not moving."""
    k, L = 31, 64
    rng = np.random.default_rng(78)
    lines = _lines(rng, 12, L)
    dev = _Dev(torch, oracle, *_batch(rng, lines, np.arange(12)), k, True)
    with rig.ctx(kmc, k) as kc:
        _planned(rig, kmc, kc, dev, "refusals")
        # one read with an N: the deferred list is not empty
        bases, offs = _batch(rng, lines, np.arange(12))
        bases[700 * L + 20] = ord("N")
        assert _cycle(rig, kc, _Dev(torch, oracle, bases, offs, k, True), tag="N")[:2] == (0, 0)
        assert _cycle(rig, kc, dev, tag="behind N")[:2] == (1, 0)
        # add, add, finalize
        f0, b0 = _counters(kc)
        kc.reset()
        rig.hold()
        dev.add(kc)
        dev.add(kc)
        want2 = _concat(oracle, [dev, dev], k, True)
        assert kc.finalize() == (want2.n_distinct, want2.n_total)
        assert kc.export().equals(want2)
        assert _counters(kc) == (f0, b0)
        assert _cycle(rig, kc, dev, tag="behind add add")[:2] == (1, 0)
    # L < k: an empty table, so no plan is built
    short = _Dev(torch, oracle, *_batch(rng, _lines(rng, 12, 16), np.arange(12)), k, True)
    assert short.want.n_distinct == 0
    with rig.ctx(kmc, k) as kc:
        for i in range(3):
            assert _cycle(rig, kc, short, tag=("short", i))[:2] == (0, 0)
    # more than 4096 distinct k-mers that still walk
    big = _Dev(torch, oracle, *_batch(rng, _lines(rng, 16, 400), np.arange(16)), k, True)
    assert big.want.n_distinct > PLAN_MAX
    with rig.ctx(kmc, k) as kc:
        for i in range(3):
            assert _cycle(rig, kc, big, tag=("big", i))[:2] == (0, 0)
        assert kc.stats().algo_last == kmc.ALGO_WALK
    # KMC_WALK_NO_PLAN=1 (read by kmc_create): the same results, no plan
    with rig.ctx(kmc, k) as kc:
        _planned(rig, kmc, kc, dev, "plan run")
        kc.finalize()
        with_plan = kc.export()
    monkeypatch.setenv("KMC_WALK_NO_PLAN", "1")
    with rig.ctx(kmc, k) as kc:
        for i in range(3):
            assert _cycle(rig, kc, dev, tag=("no plan", i))[:2] == (0, 0)
        assert kc.export().equals(with_plan)


def test_orderings_around_a_plan_finalize(kmc, oracle, torch, rig):
    k, L = 31, 64
    rng = np.random.default_rng(79)
    lines = _lines(rng, 12, L)
    dev = _Dev(torch, oracle, *_batch(rng, lines, np.arange(12)), k, True)
    want2 = _concat(oracle, [dev, dev], k, True)
    kd = importlib.import_module("k-mer-count_amd.distributed")

    def dev_u64(ptr, n):
        return kd.device_view(ptr, n, torch.device("cuda", 0)).cpu().numpy().view(np.uint64).copy()

    with rig.ctx(kmc, k) as kc:
        _planned(rig, kmc, kc, dev, "orderings")
        # add, finalize, add, finalize: undrain behind a plan-made view
        f0, _ = _counters(kc)
        kc.reset(); rig.hold(); dev.add(kc)
        assert kc.finalize() == (dev.want.n_distinct, dev.want.n_total)
        assert _counters(kc)[0] == f0 + 1
        dev.add(kc)
        assert kc.finalize() == (want2.n_distinct, want2.n_total) and kc.export().equals(want2)
        assert _counters(kc)[0] == f0 + 1
        # add, finalize_async, add
        kc.reset(); rig.hold(); dev.add(kc)
        kc.finalize_async()
        dev.add(kc)
        assert kc.finalize() == (want2.n_distinct, want2.n_total) and kc.export().equals(want2)
        assert _counters(kc)[0] == f0 + 2
        # add, finalize_async, reset, add, finalize
        kc.reset(); rig.hold(); dev.add(kc)
        kc.finalize_async()
        assert _cycle(rig, kc, dev, tag="behind async + reset")[0] == 1
        # export_device and export straight after a plan finalize
        f1, _ = _counters(kc)
        kc.reset(); rig.hold(); dev.add(kc)
        kc.finalize()
        assert _counters(kc)[0] == f1 + 1
        _, dlo, dcnt, n = kc.export_device()
        assert n == dev.want.n_distinct
        assert np.array_equal(dev_u64(dlo, n), dev.want.key_lo) and np.array_equal(dev_u64(dcnt, n), dev.want.count)
        assert kc.export().equals(dev.want)
        # forget_source(memo=True) between cycles: the plan goes with the memo and comes back with it
        kc.forget_source(memo=True)
        _planned(rig, kmc, kc, dev, "behind forget")
    # two contexts on one device (two streams), cycles interleaved; the second one on a side stream of its own
    other = _Dev(torch, oracle, *_batch(rng, _lines(rng, 12, 400), np.arange(12)), 63, False)
    side = torch.cuda.Stream()
    with rig.ctx(kmc, k) as ka, rig.ctx(kmc, 63, canonical=False, stream=side) as kb:
        for cyc in range(1, 5):
            fa = _cycle(rig, ka, dev, tag=("a", cyc))[0]
            fb = _cycle(rig, kb, other, tag=("b", cyc), stream=side)[0]
            assert (fa, fb) == ((1, 1) if cyc >= 2 else (0, 0)), (cyc, fa, fb)
    # a ctx on its own stream, and a one-read batch: either path may win the race with the request -- exact either way
    one = _Dev(torch, oracle, *_batch(rng, lines, np.arange(1), n_reads=1), k, True)
    with kmc.KmerCounter(k=k, algo=kmc.ALGO_WALK) as kc:
        for cyc in range(4):
            kc.reset(); dev.add(kc)
            assert kc.finalize() == (dev.want.n_distinct, dev.want.n_total) and kc.export().equals(dev.want)
        for cyc in range(4):
            kc.reset(); one.add(kc)
            assert kc.finalize() == (one.want.n_distinct, one.want.n_total) and kc.export().equals(one.want)


def test_random_call_sequences(kmc, oracle, torch, rig):
    """Seeded random sequences of reset / add / finalize / finalize_async / export / forget_source over three pool batches
    of one source, against a host model of everything added since the last reset."""
    k, L = 31, 64
    rng = np.random.default_rng(20261020)
    lines = _lines(rng, 16, L)
    devs = [_Dev(torch, oracle, *_batch(rng, lines, w), k, True) for w in (np.arange(12), np.arange(4, 16), np.arange(8))]
    tables = {}

    def want_of(held):
        key = tuple(sorted(held))
        if key not in tables:
            tables[key] = _concat(oracle, [devs[i] for i in key], k, True)
        return tables[key]

    with rig.ctx(kmc, k) as kc:
        held = []
        kc.reset()
        for op_i in range(160):
            r = rng.random()
            if not held or r < 0.35:
                if held and rng.random() < 0.8:
                    kc.reset()
                    held = []
                i = int(rng.integers(0, 3)) if rng.random() < 0.3 else 0
                rig.hold()
                devs[i].add(kc)
                held.append(i)
            elif r < 0.70:
                w = want_of(held)
                assert kc.finalize() == (w.n_distinct, w.n_total), (op_i, held)
            elif r < 0.82:
                kc.finalize_async()
            elif r < 0.94:
                assert kc.export().equals(want_of(held)), (op_i, held)
            elif r < 0.97:
                kc.forget_source(memo=True)
            else:
                kc.reset()
                held = []
        assert kc.export().equals(want_of(held)) if held else True
        f, b = _counters(kc)
        print("random sequences: plan finalizes", f, "builds", b)
        assert f >= 1 and b >= 1
