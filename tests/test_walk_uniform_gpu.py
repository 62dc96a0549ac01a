"""Batches whose reads all have one length L <= 416: the walk kernels compute the reads' bounds (read r = bases
[r * L, (r + 1) * L)) and load no offsets.  Every case is compared with the CPU oracle through Table.equals, and
kmc_stats.walk_uniform_launches proves which variant ran: it grows by launches_last when the batch was uniform and
does not move otherwise.  The batches go through kmc_add_batch_device, once with max_read_len = L and once with 0
(the maximum is then computed on the device)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)
LENGTHS = (1, 15, 16, 17, 31, 33, 64, 150, 399, 400, 401, 416)
KS = (5, 21, 31, 32, 33, 63)
N_READS = (1, 64, 65, 1500)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "the gpu tests need a GPU"
    return t


def _uniform_batch(rng, n_reads, L, kind):
    """n_reads reads of L bases.  'pool': every read is one of a dozen lines (the memo's hot path carries them);
    'random': independent bases (steps fall off the memo)."""
    if kind == "pool":
        pool = ACGT[rng.integers(0, 4, (12, L))]
        bases = pool[rng.integers(0, 12, n_reads)].reshape(-1).copy()
    else:
        bases = ACGT[rng.integers(0, 4, n_reads * L)].copy()
    offs = (np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(L))
    return bases, offs


def _ragged_batch(rng, n_reads, lo, hi):
    lens = rng.integers(lo, hi + 1, n_reads)
    offs = np.zeros(n_reads + 1, np.uint64)
    offs[1:] = np.cumsum(lens)
    return ACGT[rng.integers(0, 4, int(offs[-1]))].copy(), offs


def _upload(torch, bases, offs):
    """Device copies; the bases are padded so that the 16-byte piece that holds the last base is readable."""
    pad = np.full(len(bases) + 16, ord("N"), np.uint8)   # (non-ACGT behind the batch: must be ignored)
    pad[:len(bases)] = bases
    return torch.from_numpy(pad).cuda(), torch.from_numpy(offs.astype(np.int64)).cuda()


def _add(kc, torch, bases, offs, max_read_len, d=None):
    """One batch through kmc_add_batch_device; returns (growth of walk_uniform_launches, stats), after the batch ran."""
    db, do = d if d is not None else _upload(torch, bases, offs)
    before = kc.stats().walk_uniform_launches
    kc.add_batch_device(db.data_ptr(), do.data_ptr(), len(offs) - 1, len(bases), max_read_len)
    kc.poll()   # (synchronises: the device buffers may go, launches_last is this batch's)
    st = kc.stats()
    return st.walk_uniform_launches - before, st


def _check_uniform(kmc, oracle, torch, kc, bases, offs, L, k, canonical, want, tag, kind="pool"):
    """launches_last counts every bracketed launch of the batch.  Once a ctx has seen steps fall off the memo (random
    reads) it logs them, and the log's counting pipeline is one more bracketed launch behind every walk launch; so that
    launches_last is the number of walk launches, a random batch and the batch after one start from a forgotten source
    (kmc_forget_source switches the log off; the memo is then cold, pool batches in a row keep it warm)."""
    d = _upload(torch, bases, offs)
    for mrl in (L, 0):
        kc.reset()
        if kind != "pool" or getattr(kc, "log_may_be_on", False):
            kc.forget_source()
        kc.log_may_be_on = kind != "pool"
        grew, st = _add(kc, torch, bases, offs, mrl, d)
        got = kc.export()
        print("uniform", tag, "mrl", mrl, "launches_last", st.launches_last, "uniform launches", grew, "algo", st.algo_last)
        assert got.equals(want), (tag, mrl)
        assert st.algo_last == kmc.ALGO_WALK and st.launches_last >= 1 and grew == st.launches_last, (tag, mrl, grew, st.launches_last)
    return got


def _boundary_cases(k):
    """(L, n_reads, canonical, kind) for this k.  The product is pruned: every L with k in {31, 63}, every k with L in
    {17, 400}; each kept (L, k) runs every n_reads once, with strand and kind of input rotating over them."""
    out = []
    for li, L in enumerate(LENGTHS):
        if not (k in (31, 63) or L in (17, 400)):
            continue
        for ni, n in enumerate(N_READS):
            r = ni + li + KS.index(k)
            out.append((L, n, r % 2 == 0, "pool" if (r // 2) % 2 == 0 else "random"))
    return out


@pytest.mark.parametrize("k", KS)
def test_boundaries(kmc, oracle, torch, k):
    """Equal-length batches at the lengths where a tile's byte range, the 16-byte pieces and the 16-base steps line up or
    just fail to (including L < k: an empty table, and L == k), 1 read to 24 tiles, both strands, pool and random reads."""
    rng = np.random.default_rng(4000 + k)
    cases = _boundary_cases(k)
    # every kind of input, strand and batch size occurs for this k
    assert {c[2] for c in cases} == {True, False} and {c[3] for c in cases} == {"pool", "random"} and {c[1] for c in cases} == set(N_READS)
    with kmc.KmerCounter(k=k, canonical=True, algo=kmc.ALGO_WALK) as kc_c, kmc.KmerCounter(k=k, canonical=False, algo=kmc.ALGO_WALK) as kc_f:
        for L, n, canonical, kind in cases:
            bases, offs = _uniform_batch(rng, n, L, kind)
            want = oracle.count_kmers(bases, offs, k, canonical)
            _check_uniform(kmc, oracle, torch, kc_c if canonical else kc_f, bases, offs, L, k, canonical, want, (L, k, n, canonical, kind), kind)


@pytest.mark.parametrize("k,L", [(31, 400), (21, 33), (63, 150), (5, 16)])
def test_non_acgt_bytes_in_uniform_batches(kmc, oracle, torch, k, L):
    """Reads with a byte outside ACGT are diverted to the scalar part of the tail kernel, which finds them by r * L too:
    N at a read's first base, its last base, in the middle; a whole read of N; a whole tile of such reads; lowercase."""
    rng = np.random.default_rng(5000 + k)
    n = 64 * 4 + 7
    bases, offs = _uniform_batch(rng, n, L, "pool")
    b = bases.reshape(n, L)
    b[3, 0] = ord("N")
    b[5, L - 1] = ord("N")
    b[6, L // 2] = ord("N")
    b[63, 0] = ord("N"); b[64, L - 1] = ord("N")      # (either side of a tile boundary)
    b[9, :] = ord("N")
    b[128:192, :] = ord("N")                           # a whole tile
    b[200, :] = np.frombuffer(b"acgt", np.uint8)[rng.integers(0, 4, L)]
    b[201, L // 3] = ord("a")
    b[n - 1, L - 1] = ord("n")                         # the batch's last base
    bases = b.reshape(-1).copy()
    for canonical in (True, False):
        want = oracle.count_kmers(bases, offs, k, canonical)
        with kmc.KmerCounter(k=k, canonical=canonical, algo=kmc.ALGO_WALK) as kc:
            _check_uniform(kmc, oracle, torch, kc, bases, offs, L, k, canonical, want, ("non-ACGT", L, k, canonical))
    # every read of every tile diverted
    bases[:] = ord("N")
    with kmc.KmerCounter(k=k, algo=kmc.ALGO_WALK) as kc:
        _check_uniform(kmc, oracle, torch, kc, bases, offs, L, k, True, oracle.count_kmers(bases, offs, k, True), ("all N", L, k))


def _check_ragged_path(kmc, torch, kc, bases, offs, mrl, want, tag):
    kc.reset()
    grew, st = _add(kc, torch, bases, offs, mrl)
    got = kc.export()
    print("not uniform", tag, "mrl", mrl, "launches_last", st.launches_last, "uniform launches", grew)
    assert got.equals(want), tag
    assert st.algo_last == kmc.ALGO_WALK and st.launches_last >= 1 and grew == 0, (tag, grew)
    return got


def test_not_uniform_still_exact_counter_does_not_move(kmc, oracle, torch, monkeypatch):
    rng = np.random.default_rng(6000)
    k = 31
    with kmc.KmerCounter(k=k, algo=kmc.ALGO_WALK) as kc:
        # a ragged batch -- one whose total is a multiple of the read count and max_read_len the true maximum included
        bases, offs = _ragged_batch(rng, 700, 0, 416)
        want = oracle.count_kmers(bases, offs, k, True)
        for mrl in (int(np.diff(offs.astype(np.int64)).max()), 0):
            _check_ragged_path(kmc, torch, kc, bases, offs, mrl, want, "ragged")
        lens = np.tile(np.array([399, 401, 400, 400], np.uint64), 50)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        bases = ACGT[rng.integers(0, 4, int(offs[-1]))].copy()
        want = oracle.count_kmers(bases, offs, k, True)
        for mrl in (401, 0):
            _check_ragged_path(kmc, torch, kc, bases, offs, mrl, want, "ragged, mean 400")
        # equal lengths above 416: walked as pieces
        for L in (417, 1000):
            bases, offs = _uniform_batch(rng, 130, L, "pool")
            want = oracle.count_kmers(bases, offs, k, True)
            for mrl in (L, 0):
                _check_ragged_path(kmc, torch, kc, bases, offs, mrl, want, ("pieces", L))
        # L = 400 under a max_read_len that is only an upper bound
        bases, offs = _uniform_batch(rng, 300, 400, "pool")
        want = oracle.count_kmers(bases, offs, k, True)
        _check_ragged_path(kmc, torch, kc, bases, offs, 416, want, "L 400 as max_read_len 416")
        # ... and the same batch is uniform when max_read_len says so
        kc.log_may_be_on = True   # (the ragged batches above were random reads)
        with_uniform = _check_uniform(kmc, oracle, torch, kc, bases, offs, 400, k, True, want, "L 400")
    monkeypatch.setenv("KMC_WALK_NO_UNIFORM", "1")
    with kmc.KmerCounter(k=k, algo=kmc.ALGO_WALK) as kc:
        for mrl in (400, 0):
            got = _check_ragged_path(kmc, torch, kc, bases, offs, mrl, want, "KMC_WALK_NO_UNIFORM=1")
            assert got.equals(with_uniform)
    monkeypatch.delenv("KMC_WALK_NO_UNIFORM")
    with kmc.KmerCounter(k=k, algo=kmc.ALGO_WALK) as kc:   # (the switch is read at kmc_create)
        _check_uniform(kmc, oracle, torch, kc, bases, offs, 400, k, True, want, "switch off again")


@pytest.mark.parametrize("k,canonical", [(31, True), (63, False)])
def test_one_ctx_uniform_and_ragged_batches_without_reset(kmc, oracle, torch, k, canonical):
    rng = np.random.default_rng(7000 + k)
    n1, h = 300, 150
    b1, o1 = _uniform_batch(rng, n1, 400, "pool")
    b2, o2 = _ragged_batch(rng, 500, 0, 416)
    b3, o3 = _uniform_batch(rng, 200, 150, "random")
    d1, d2, d3 = _upload(torch, b1, o1), _upload(torch, b2, o2), _upload(torch, b3, o3)
    o4 = o1[h:] - o1[h]                                   # the second half of batch 1, rebased
    d4 = (d1[0][h * 400:], torch.from_numpy(o4.astype(np.int64)).cuda())
    assert d4[0].data_ptr() == d1[0].data_ptr() + h * 400 and d4[0].data_ptr() % 16 == 0
    with kmc.KmerCounter(k=k, canonical=canonical, algo=kmc.ALGO_WALK) as kc:
        g1, s1 = _add(kc, torch, b1, o1, 400, d1)
        g2, s2 = _add(kc, torch, b2, o2, 0, d2)
        g3, s3 = _add(kc, torch, b3, o3, 0, d3)
        g4, s4 = _add(kc, torch, b1[h * 400:], o4, 400, d4)
        got = kc.export()
    # (batches 2 and 3 are random reads: from then on the log pipeline's launches are part of launches_last)
    assert g1 == s1.launches_last and g2 == 0 and 1 <= g3 <= s3.launches_last and 1 <= g4 <= s4.launches_last, (g1, g2, g3, g4)
    allb = np.concatenate([b1, b2, b3, b1[h * 400:]])
    allo = np.concatenate([o1, o1[-1] + o2[1:], o1[-1] + o2[-1] + o3[1:], o1[-1] + o2[-1] + o3[-1] + o4[1:]]).astype(np.uint64)
    assert got.equals(oracle.count_kmers(allb, allo, k, canonical))


def test_several_launches_per_batch(kmc, oracle, torch):
    """A fresh ctx has no history and a table of the smallest size (capacity_hint = 1): its first launch takes only the 33
    tiles of 64 x 400 bases whose k-mers fit for certain, the rest of the batch goes out in further launches, which
    start at tile_begin != 0."""
    rng = np.random.default_rng(8000)
    bases, offs = _uniform_batch(rng, 64 * 80 + 5, 400, "pool")
    want = oracle.count_kmers(bases, offs, 31, True)
    for mrl in (400, 0):
        with kmc.KmerCounter(k=31, algo=kmc.ALGO_WALK, capacity_hint=1) as kc:
            grew, st = _add(kc, torch, bases, offs, mrl)
            got = kc.export()
        print("several launches: launches_last", st.launches_last, "uniform", grew)
        assert got.equals(want)
        # (launches_last also brackets the (k+16)-mer unfold the planner queues in front of a launch sized by a prediction:
        #  what has to be two or more is the walk launches themselves, and every one of them uniform)
        assert st.launches_last >= 2 and 2 <= grew <= st.launches_last, (grew, st.launches_last)
