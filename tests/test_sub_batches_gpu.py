"""The sub-batch seams of the sort path and of LR mode, crossed on inputs the CPU oracle can count.

run_sort_path sorts at most 2^21 chunks (2^31 base positions) per pass and count_lr forms the keys of at most 2^25
window starts per pass.  Everything behind the first pass is index arithmetic relative to a moving origin -- the
extraction's `cb - chunk_begin * KMC_CHUNK`, the histogram rows of a later range, `rank[P0 + i - q0]`, the 64-ary search
for the read of a pass's first start, a dictionary of 27-mers per pass -- and is trivially right while the origin is 0,
which it is for every input below tens of gigabytes.  KMC_SORT_SUB_CHUNKS and KMC_LR_SUB_STARTS (read once in kmc_create)
turn the two constants down to 64..192 chunks and 256..4096 starts, the smallest values at which the arithmetic is still
legal, so that a batch of half a million bases crosses three to eight edges.  Every comparison is the whole table against
the oracle, exact.

Proof that a seam engaged: every pass brackets its launches with an event pair of its own, so kmc_stats.launches_last
(launches_lifetime where a ctx takes several batches) is at least the number of passes the seam implies.  With the seam
not engaged a sort-path batch has two brackets (extraction, sort) and an LR batch one, so the cases here have at least
three passes (sort) or two (LR).

The whole-file fallback (count_file_whole, batches of 2^30 bases) has no test and no seam: it is entered only for a path
that opens but is not a regular file or cannot be mapped, and it then sizes the file with fseeko / ftello and parses
segments of it by offset from several threads, each opening the path again -- a FIFO is opened several times and never
delivers its bytes to the parser, so no such input exists without changing the reader.

Cost on one MI355X: 11 s for the file (57 cases; the recovery case takes 2.7 s of it, the leaf-size case 1.1 s).
"""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, SAMPLE

pytestmark = pytest.mark.gpu

LR = json.load(open(os.path.join(GOLDEN, "lr_goldens.json")))["cases"]
CHUNK = 1024                  # KMC_CHUNK: base positions per chunk
RANGE = 65536                 # KMC_MSD_RANGE: keys per range of the sort (64 chunks)
SORT_SUBS = (64, 128, 192)    # KMC_SORT_SUB_CHUNKS
LR_SUBS = (256, 512, 4096)    # KMC_LR_SUB_STARTS
EDGE = 64 * CHUNK             # every edge of the three sort seams is a multiple of this
N_SORT = 500_003              # bases of a one-batch sort case: 8, 4 and 3 passes
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _rand(rng, n):
    return ACGT[rng.integers(0, 4, int(n))].copy()


def _offs(lens):
    o = np.zeros(len(lens) + 1, np.uint64)
    o[1:] = np.cumsum(np.asarray(lens, dtype=np.uint64))
    return o


def _ragged(rng, total, lo, hi):
    """Offsets of reads of lo..hi bases, `total` bases in all."""
    lens, s = [], 0
    while s < total:
        l = min(int(rng.integers(lo, hi + 1)), total - s)
        lens.append(l)
        s += l
    return _offs(lens)


def _cut(bases, offs, r0, r1):
    a, b = int(offs[r0]), int(offs[r1])
    return bases[a:b], offs[r0:r1 + 1] - offs[r0]


# ---- the sort path ----------------------------------------------------------------------------------------------------
def _sort_passes(n_bases, sub):
    n_chunks = (n_bases + CHUNK - 1) // CHUNK
    return (n_chunks + sub - 1) // sub


def _check_sort(kmc, monkeypatch, want, k, canonical, bases, offs, subs=SORT_SUBS):
    for sub in subs:
        monkeypatch.setenv("KMC_SORT_SUB_CHUNKS", str(sub))
        passes = _sort_passes(int(offs[-1]), sub)
        assert passes >= 3
        with kmc.KmerCounter(k=k, canonical=canonical, algo=kmc.ALGO_SORT) as kc:
            kc.add_batch(bases, offs)
            t = kc.export()
            st = kc.stats()
        assert st.algo_last == kmc.ALGO_SORT, (k, canonical, sub)
        assert st.launches_last >= passes, (k, canonical, sub, st.launches_last, passes)
        assert t.equals(want) and t.n_total == want.n_total, (k, canonical, sub, t.n_distinct, want.n_distinct, t.n_total, want.n_total)


K_CANON = [(k, c) for k in (1, 5, 31, 32, 63) for c in (True, False)]


@pytest.mark.parametrize("k,canonical", K_CANON)
def test_sort_one_read_across_every_edge(kmc, oracle, monkeypatch, k, canonical):
    """One read spans the batch: k - 1 windows straddle every edge, and the halo of a pass's first chunk is the last chunk
    of the pass before."""
    bases = _rand(np.random.default_rng(100 + k), N_SORT)
    offs = np.array([0, N_SORT], np.uint64)
    _check_sort(kmc, monkeypatch, oracle.count_kmers(bases, offs, k, canonical, method=1), k, canonical, bases, offs)


@pytest.mark.parametrize("k,canonical", K_CANON)
def test_sort_reads_end_around_every_edge(kmc, oracle, monkeypatch, k, canonical):
    """Reads end at edge - k + 1, edge - 1, edge, edge + 1 and edge + k - 1 for every edge, with an empty read at the edge
    and one behind it: the first window of a pass is the last one of a read, the first one of the next, or none."""
    ends = []
    for e in range(EDGE, N_SORT, EDGE):
        ends += [e - k + 1, e - 1, e, e, e + 1, e + 1, e + k - 1]
    ends = sorted(x for x in ends if 0 < x < N_SORT)
    offs = np.array([0] + ends + [N_SORT, N_SORT], np.uint64)   # (and a trailing empty read)
    assert (np.diff(offs.astype(np.int64)) == 0).sum() >= 2 * (N_SORT // EDGE)
    bases = _rand(np.random.default_rng(200 + k), N_SORT)
    _check_sort(kmc, monkeypatch, oracle.count_kmers(bases, offs, k, canonical, method=1), k, canonical, bases, offs)


@pytest.mark.parametrize("k", [5, 31, 63])
def test_sort_ragged_reads_bad_bytes_at_edges(kmc, oracle, monkeypatch, k):
    """Reads of 0 to 3000 bases, and N bytes within k bases on either side of every edge: the windows a bad byte spoils
    reach from one pass into the next."""
    rng = np.random.default_rng(300 + k)
    offs = _ragged(rng, N_SORT, 0, 3000)
    bases = _rand(rng, N_SORT)
    where = [(-k, k - 1), (-1,), (0,), (1, -k + 1), (k,), (-(k // 2) - 1, k // 2), (-1, 0, 1)]
    for i, e in enumerate(range(EDGE, N_SORT, EDGE)):
        for d in where[i % len(where)]:
            bases[e + d] = ord("N")
    assert N_SORT // EDGE >= len(where)
    _check_sort(kmc, monkeypatch, oracle.count_kmers(bases, offs, k, True, method=1), k, True, bases, offs)


@pytest.mark.parametrize("k,canonical,pool", [(31, True, 10), (63, True, 10), (32, False, 10), (31, True, 0), (63, False, 0)])
def test_sort_runs_share_keys_or_share_none(kmc, oracle, monkeypatch, k, canonical, pool):
    """Lines from a pool of ten: every pass leaves a run with the same few thousand keys, and the weighted merge of
    kmc_finalize sums each key over all runs.  Pool 0: random reads, all keys distinct, every run as long as its pass."""
    bases, offs = kmc.synth_reads_host(kmc.Synth(seed=400 + k, pool=pool), 0, N_SORT // 400 + 1)
    want = oracle.count_kmers(bases, offs, k, canonical, method=1)
    if pool:
        assert want.n_total >= 50 * want.n_distinct
    else:
        assert want.n_total <= want.n_distinct + 8
    _check_sort(kmc, monkeypatch, want, k, canonical, bases, offs)


def _simulate_acc(sub, batch_bases, acc=0):
    """run_sort_path's accumulator over these batches: (extractions, flushes in the middle of the run, flushes that
    sorted keys of an EARLIER batch together with the current one's, keys left unsorted)."""
    cap = sub * CHUNK
    ext = flushes = carried = 0
    for nb in batch_bases:
        n_chunks = (nb + CHUNK - 1) // CHUNK
        earlier = acc > 0
        for cb in range(0, n_chunks, sub):
            n = (min(n_chunks, cb + sub) - cb + 63) // 64 * RANGE
            if acc + n > cap and acc:
                flushes += 1
                carried += 1 if earlier else 0
                earlier = False
                acc = 0
            ext += 1
            acc += n
    return ext, flushes, carried, acc


MULTI = [  # (seam, k, bases of the batches before the first finalize, bases of the batch after it)
    (192, 31, [30_000, 70_000, 30_000, 200_000, 10_000], 40_000),
    (128, 31, [70_000, 70_000, 70_000, 150_000], 50_000),
    (64, 31, [100_000, 30_000, 200_000], 70_000),
    (192, 63, [30_000, 70_000, 30_000, 200_000, 10_000], 40_000),
]


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("sub,k,first,last", MULTI)
def test_sort_flush_with_keys_of_an_earlier_batch(kmc, oracle, monkeypatch, sub, k, first, last, device):
    """Several batches on one ctx: the accumulator is flushed while it still holds an earlier batch's keys, a batch is
    cut by a flush in its middle, and after a finalize (a stale view, runs) one more batch arrives.  Host batches and
    device batches with max_read_len 0.  The oracle's table of the concatenation, at the finalize in the middle and at
    the end."""
    torch = pytest.importorskip("torch") if device else None
    rng = np.random.default_rng(500 + sub + k)
    total = sum(first) + last
    offs = _ragged(rng, total, 0, 600)
    bases = _rand(rng, total)
    targets = np.cumsum(first + [last])
    cuts = [0] + [int(np.searchsorted(offs, t, side="left")) for t in targets]
    cuts[-1] = offs.shape[0] - 1
    parts = [_cut(bases, offs, a, b) for a, b in zip(cuts[:-1], cuts[1:])]
    sizes = [int(o[-1]) for _, o in parts]
    ext, flushes, carried, left = _simulate_acc(sub, sizes[:-1])
    assert carried >= 1 and left > 0
    ext2, flushes2, _, left2 = _simulate_acc(sub, sizes[-1:])
    assert left2 > 0
    implied = ext + flushes + 1 + ext2 + flushes2 + 1       # (+ 1: each finalize sorts what is left)
    assert implied > len(parts) + 2 + 2                      # seam not engaged: one extraction per batch, two sorts, two merges
    mid = int(offs[cuts[-2]])
    want_mid = oracle.count_kmers(bases[:mid], offs[:cuts[-2] + 1], k, True, method=1)
    want_all = oracle.count_kmers(bases, offs, k, True, method=1)
    monkeypatch.setenv("KMC_SORT_SUB_CHUNKS", str(sub))
    keep = []

    def add(kc, b, o):
        if not device:
            kc.add_batch(b, o)
            return
        d_b = torch.from_numpy(np.concatenate([b, np.zeros(64, np.uint8)])).cuda()
        d_o = torch.from_numpy(o.astype(np.int64)).cuda()
        torch.cuda.synchronize()
        keep.append((d_b, d_o))
        kc.add_batch_device(d_b.data_ptr(), d_o.data_ptr(), o.shape[0] - 1, int(o[-1]), 0)

    with kmc.KmerCounter(k=k, algo=kmc.ALGO_SORT) as kc:
        for b, o in parts[:-1]:
            add(kc, b, o)
        t = kc.export()
        assert t.equals(want_mid), (sub, k, device, "first finalize", t.n_total, want_mid.n_total)
        add(kc, *parts[-1])
        t = kc.export()
        st = kc.stats()
        assert t.equals(want_all), (sub, k, device, "runs + a new batch", t.n_total, want_all.n_total)
        assert st.algo_last == kmc.ALGO_SORT and st.n_batches == len(parts)
        assert st.launches_lifetime >= implied, (sub, k, device, st.launches_lifetime, implied)
        assert kc.export().equals(want_all)                  # (nothing new: the same view)


def test_sort_recovery_enters_behind_the_start_and_crosses_edges(kmc, oracle, monkeypatch):
    """As test_wrong_prediction_is_recovered_not_fatal, one batch: a long run of N and repeats, then random reads.  The
    walk path's oversized launch is undone and run_sort_path counts the rest of the batch from the launch's first base:
    range_begin > 0, the first pass starts in the middle of a chunk's worth of windows that belong to the launches
    before, and with the seam at 64 chunks the loop crosses edges behind it.  The seam engaged if the batch has more
    launches than the same batch on a ctx without it (the walk launches are the same; the sort path adds two per pass)."""
    k = 31
    lo_b, lo_o = kmc.synth_reads_host(kmc.Synth(seed=21, pool=10), 0, 300_000)
    hi_b, hi_o = kmc.synth_reads_host(kmc.Synth(seed=22, pool=0), 0, 12_000)
    want = oracle.count_kmers(np.concatenate([lo_b, hi_b]), np.concatenate([lo_o, hi_o[1:] + lo_o[-1]]), k, True, method=1)
    n_b = np.full(400 * 50_000, ord("N"), np.uint8)
    n_o = np.arange(50_001, dtype=np.uint64) * np.uint64(400)
    mix_b = np.concatenate([n_b, lo_b, hi_b])
    mix_o = np.concatenate([n_o, lo_o[1:] + n_o[-1], hi_o[1:] + n_o[-1] + lo_o[-1]])
    launches = {}
    for sub in (None, 64):
        if sub:
            monkeypatch.setenv("KMC_SORT_SUB_CHUNKS", str(sub))
        else:
            monkeypatch.delenv("KMC_SORT_SUB_CHUNKS", raising=False)
        with kmc.KmerCounter(k=k, algo=kmc.ALGO_WALK) as kc:
            kc.forget_source(memo=True, history=True)
            kc.add_batch(mix_b, mix_o)
            t = kc.export()
            st = kc.stats()
        assert t.equals(want), (sub, t.n_total, want.n_total)
        assert st.algo_last == kmc.ALGO_SORT, sub             # (a WALK ctx reports SORT only after a recovery)
        launches[sub] = st.launches_last
    # at least two edges behind the point of entry: three passes where the ctx without the seam has one
    assert launches[64] >= launches[None] + 2 * 2, launches


def test_sort_two_word_keys_both_leaf_sizes(kmc, oracle, monkeypatch):
    """k = 63 as test_two_word_sort_with_both_leaf_sizes: a repetitive batch, the same again, a random one.

    With the seam at 64 a sort has at most 65536 keys, and the switch to leaves of 1024 keys needs an unweighted sort of
    2^20 valid keys that collapses fourfold (msd_sort_to_run: msd_dup_heavy): such a ctx sorts with leaves of 2048 keys
    only, which is what the first half checks.  The second half reaches both leaf sizes ACROSS an edge at the smallest
    seam that allows it, 1280 chunks (1.31 M positions, 1.1 M valid 63-mers of reads of 400 bases): the first pass of
    the repetitive batch sets the flag, its later passes and the next batch's first pass sort with leaves of 1024, the
    random batch's first pass clears it.  That takes batches of 3.6 M bases, three passes each."""
    k = 63
    for sub, n_rec in ((64, 1500), (1280, 9000)):
        rep_b, rep_o = kmc.synth_reads_host(kmc.Synth(seed=5, pool=40), 0, n_rec)
        rnd_b, rnd_o = kmc.synth_reads_host(kmc.Synth(seed=6, pool=0), 0, n_rec)
        want_rep = oracle.count_kmers(rep_b, rep_o, k, True, method=1)
        want_rnd = oracle.count_kmers(rnd_b, rnd_o, k, True, method=1)
        passes = _sort_passes(n_rec * 400, sub)
        assert passes >= 3
        if sub == 1280:
            assert sub * CHUNK * 338 // 400 >= (1 << 20) and want_rep.n_total >= 4 * want_rep.n_distinct
        monkeypatch.setenv("KMC_SORT_SUB_CHUNKS", str(sub))
        with kmc.KmerCounter(k=k, algo=kmc.ALGO_SORT) as kc:
            for hb, ho, want in ((rep_b, rep_o, want_rep), (rep_b, rep_o, want_rep), (rnd_b, rnd_o, want_rnd), (rnd_b, rnd_o, want_rnd)):
                kc.reset()
                kc.add_batch(hb, ho)
                t = kc.export()
                st = kc.stats()
                assert t.equals(want), (sub, t.n_total, want.n_total)
                assert st.algo_last == kmc.ALGO_SORT and st.launches_last >= passes, (sub, st.launches_last, passes)


# ---- LR mode ----------------------------------------------------------------------------------------------------------
def _lr_passes(n_bases, sub):
    return (n_bases + sub - 1) // sub


def _check_lr(kmc, monkeypatch, want, bases, offs, subs=LR_SUBS):
    for sub in subs:
        monkeypatch.setenv("KMC_LR_SUB_STARTS", str(sub))
        passes = _lr_passes(int(offs[-1]), sub)
        assert passes >= 2
        with kmc.KmerCounter(mode=kmc.MODE_LR) as kc:
            kc.add_batch(bases, offs)
            t = kc.export()
            st = kc.stats()
        assert st.launches_last >= passes, (sub, st.launches_last, passes)
        assert t.equals(want) and t.n_total == want.n_total, (sub, t.n_distinct, want.n_distinct, t.n_total, want.n_total)


def _lr_raises(kmc, monkeypatch, sub, bases, offs, what):
    monkeypatch.setenv("KMC_LR_SUB_STARTS", str(sub))
    passes = _lr_passes(int(offs[-1]), sub)
    assert passes >= 2
    with kmc.KmerCounter(mode=kmc.MODE_LR) as kc:
        kc.add_batch(bases, offs)
        with pytest.raises(kmc.KmcError) as e:
            kc.finalize()
        assert e.value.status == kmc.ERR_ALPHABET, (sub, what)
        st = kc.stats()
    assert st.launches_last >= passes, (sub, what, st.launches_last, passes)


def test_lr_ragged_reads(kmc, oracle, monkeypatch):
    """Reads of 0 to 400 bases, 30 k bases: most reads begin in one pass and end in the next at 256 starts."""
    rng = np.random.default_rng(600)
    offs = _ragged(rng, 30_011, 0, 400)
    bases = _rand(rng, 30_011)
    _check_lr(kmc, monkeypatch, oracle.count_lr(bases, offs), bases, offs)


def test_lr_long_reads_span_several_passes(kmc, oracle, monkeypatch):
    """Reads of 1000 to 3000 bases: the read of a pass's first start began several passes earlier (the 64-ary search
    lands on the same read pass after pass), and its end lies passes ahead."""
    rng = np.random.default_rng(601)
    offs = _ragged(rng, 30_000, 1000, 3000)
    bases = _rand(rng, 30_000)
    _check_lr(kmc, monkeypatch, oracle.count_lr(bases, offs), bases, offs)


@pytest.mark.parametrize("sub", LR_SUBS)
def test_lr_reads_end_around_every_edge(kmc, oracle, monkeypatch, sub):
    """Read ends at edge - 140, - 80, - 79, - 1, edge and edge + 1: a read whose last start is the last of a pass, whose
    right 27-mers all come from the rank window's tail behind the pass (q1 = p1 + 113), that is one base too short to
    have a window in the pass at all.  At 256 starts the six ends take turns (all six at every seventh edge), so that
    reads stay long enough to have windows; at the wider seams every edge has all six."""
    n = 30_000 if sub < 4096 else 40_000
    deltas = (-140, -80, -79, -1, 0, 1)
    ends = set()
    for i, e in enumerate(range(sub, n, sub)):
        if sub >= 512 or i % 7 == 3:
            ends.update(e + d for d in deltas)
        else:
            ends.add(e + deltas[i % 6])
    offs = np.array([0] + sorted(x for x in ends if 0 < x < n) + [n], np.uint64)
    bases = _rand(np.random.default_rng(602 + sub), n)
    want = oracle.count_lr(bases, offs)
    assert want.n_total > 0
    _check_lr(kmc, monkeypatch, want, bases, offs, subs=(sub,))


@pytest.mark.parametrize("n_empty", [0, 300, 3000])
def test_lr_runs_of_empty_reads_across_edges(kmc, oracle, monkeypatch, n_empty):
    """As test_reference_mode_empty_and_short_reads, in passes: runs of up to n_empty empty reads between reads of 0..79
    and 80..400 bases.  More than 256 read ends within a workgroup's 256 starts take the pair kernel's general search,
    here with P0 > 0 and from a first read (s_first) found by the 64-ary search among thousands of equal offsets; one
    run sits exactly on an edge of all three seams."""
    rng = np.random.default_rng(610 + n_empty)
    lens = []
    for _ in range(80):
        lens.append(int(rng.integers(80, 401)))
        lens.extend([0] * int(rng.integers(0, n_empty + 1)))
        lens.append(int(rng.integers(0, 80)))
    offs = _offs(lens)
    # one run of empty reads exactly at 4096 (an edge of 256, 512 and 4096): the read that spans 4096 ends there
    i = int(np.searchsorted(offs, 4096, side="left"))
    offs = np.concatenate([offs[:i], np.full(n_empty + 1, 4096, np.uint64), offs[i:]])
    bases = _rand(rng, int(offs[-1]))
    bases[300:900] = bases[1300:1900]
    assert 20_000 <= int(offs[-1]) <= 40_000
    _check_lr(kmc, monkeypatch, oracle.count_lr(bases, offs), bases, offs)


def test_lr_equal_keys_from_different_dictionaries(kmc, oracle, monkeypatch):
    """The same stretches of bases in different passes: equal 108-bit keys are composed from different dictionaries of
    27-mers with different rank widths B (a pass of random bases next to passes of a single repeated 27-mer), and the
    merge must sum them.  Also reads drawn from a pool of five lines."""
    rng = np.random.default_rng(620)
    s = _rand(rng, 700)
    poly = np.full(1500, ord("A"), np.uint8)               # one 27-mer: B = 1 where a pass sees nothing else
    pool = [_rand(rng, 300) for _ in range(5)]
    reads = [s, _rand(rng, 1000), s, poly, _rand(rng, 3000), s[:400], poly[:200], s[100:], _rand(rng, 5000), s, poly]
    reads += [pool[int(i)] for i in rng.integers(0, 5, 40)]
    reads += [s, _rand(rng, 977), s]
    offs = _offs([r.shape[0] for r in reads])
    bases = np.concatenate(reads)
    assert 20_000 <= bases.shape[0] <= 40_000
    want = oracle.count_lr(bases, offs)
    assert want.n_total >= 2 * want.n_distinct
    _check_lr(kmc, monkeypatch, want, bases, offs)


def test_lr_sample_fasta_in_passes(kmc, oracle, monkeypatch):
    """The reference's fixture whole at 4096 starts (20 passes): the digest of the reference's own output."""
    bases, offs = kmc.parse_fasta(SAMPLE)
    monkeypatch.setenv("KMC_LR_SUB_STARTS", "4096")
    passes = _lr_passes(int(offs[-1]), 4096)
    assert passes >= 15
    with kmc.KmerCounter(mode=kmc.MODE_LR) as kc:
        kc.add_batch(bases, offs)
        t = kc.export()
        st = kc.stats()
    assert st.launches_last >= passes, (st.launches_last, passes)
    assert (t.n_distinct, t.n_total) == (LR["G-full"]["distinct"], LR["G-full"]["lines"])
    assert t.digest(expand=True) == LR["G-full"]["sha256"]


def _lr_layout(sub, n_total, special):
    """Reads of 150 random bases up to n_total, with the reads of `special` -- {start: (length, [N positions in the read])}
    -- laid in at their positions (the read in front is cut short).  Returns (bases, offs)."""
    rng = np.random.default_rng(630 + sub)
    starts, pos = [], 0
    marks = sorted(special)
    while pos < n_total:
        starts.append(pos)
        nxt = pos + (special[pos][0] if pos in special else 150)
        ahead = [m for m in marks if pos < m < nxt]
        pos = min([nxt, n_total] + ahead)
    offs = np.array(starts + [n_total], np.uint64)
    bases = _rand(rng, n_total)
    for s0, (_, ns) in special.items():
        for x in ns:
            bases[s0 + x] = ord("N")
    return bases, offs


@pytest.mark.parametrize("sub", LR_SUBS)
def test_lr_bad_byte_that_no_window_reads_is_accepted(kmc, oracle, monkeypatch, sub):
    """An N in the gap of a read of exactly 80 bases and in a read shorter than 80, both in a late pass: no chunk covers
    them (main.rs:17-23 looks at emitted chunks only), so the table is the oracle's."""
    n = 8 * sub + 200
    a = 6 * sub + 10
    special = {a: (80, [40]), a + 80: (60, [5]), 7 * sub - 30: (80, [27, 52])}   # (the third read straddles an edge)
    bases, offs = _lr_layout(sub, n, special)
    for s0, (l, _) in special.items():
        i = int(np.searchsorted(offs, s0))
        assert int(offs[i]) == s0 and int(offs[i + 1]) == s0 + l
    want = oracle.count_lr(bases, offs)
    assert want.n_total > 0
    _check_lr(kmc, monkeypatch, want, bases, offs, subs=(sub,))


@pytest.mark.parametrize("sub", LR_SUBS)
def test_lr_bad_byte_in_an_emitted_chunk_is_an_error(kmc, monkeypatch, sub):
    """ERR_ALPHABET at finalize for an N that a chunk covers: in the last pass only; in the first base of a read that
    starts exactly on an edge (the pass before ranks that position too, but forms no key from it); in the first base of
    a read that starts one base in front of an edge (only the pass's last start reads it); in the last base of a read of
    80 bases that starts there (its one window starts on the last start of a pass, and its right 27-mer lies in the
    tail of the rank window behind the pass)."""
    n = 8 * sub + 200
    cases = {
        "last pass": {n - 150: (150, [100])},
        "first base on an edge": {5 * sub: (150, [0])},
        "first base in front of an edge": {5 * sub - 1: (150, [0])},
        "right 27-mer behind the pass": {5 * sub - 1: (80, [79])},
    }
    for what, special in cases.items():
        bases, offs = _lr_layout(sub, n, special)
        s0, (l, _) = next(iter(special.items()))
        i = int(np.searchsorted(offs, s0))
        assert int(offs[i]) == s0 and int(offs[i + 1]) == s0 + l, what
        _lr_raises(kmc, monkeypatch, sub, bases, offs, what)


@pytest.mark.parametrize("sub", LR_SUBS)
def test_lr_pass_without_a_valid_27mer_is_an_error(kmc, monkeypatch, sub):
    """A read of 100 N bases that is the whole last pass: the pass's dictionary of 27-mers is empty, and its windows
    must still raise ERR_ALPHABET (the oracle and the reference abort on them).  count_lr skipped the pair kernel for a
    pass with an empty dictionary, so such a read -- or a batch of nothing else, with no seam set -- came out as an
    empty table without an error."""
    n = 8 * sub + 100
    bases, offs = _lr_layout(sub, n, {8 * sub: (100, list(range(100)))})
    assert int(offs[-2]) == 8 * sub and bytes(bases[8 * sub:]) == b"N" * 100
    _lr_raises(kmc, monkeypatch, sub, bases, offs, "last pass is one read of N")
    # the same without a seam: the batch is that read alone (one pass)
    monkeypatch.delenv("KMC_LR_SUB_STARTS")
    with kmc.KmerCounter(mode=kmc.MODE_LR) as kc:
        kc.add_batch(bases[8 * sub:], np.array([0, 100], np.uint64))
        with pytest.raises(kmc.KmcError) as e:
            kc.finalize()
        assert e.value.status == kmc.ERR_ALPHABET
    # ... and a read of N too short for a window is no error
    with kmc.KmerCounter(mode=kmc.MODE_LR) as kc:
        kc.add_batch(bases[8 * sub:8 * sub + 79], np.array([0, 79], np.uint64))
        assert kc.export().n_distinct == 0
