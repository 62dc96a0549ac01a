"""GPU checks of kmc_correct / kmc_correct_device / KmerCounter.correct_reads (kmc_correct.hip.h).  Expected values come from
tests/correct_model.py -- the definitions of include/kmc.h on Python strings -- applied to the CPU oracle's table of the
same input.  All comparisons are exact, entry by entry, through every form of the call."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import bubble_model as bm
import correct_inputs as ci
import correct_model as cm
import graph_model as gm
from conftest import ROOT, SAMPLE
from test_unitig_gpu import _dev_bytes, _dev_u64, _table_dict

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "bin", "k-mer-count")
U64, U32, U8 = np.uint64, np.uint32, np.uint8
RANGES = ((1, 0), (2, 0), (2, 3))
NAMES = ("bases", "stats", "cand_offsets", "cands")


def _want(m):
    return (np.frombuffer("".join(m.corrected).encode(), U8), np.array(m.stats, U32).reshape(-1, 4), np.array(m.cand_offsets, U64),
            np.array(m.cands, U32).reshape(-1, 4))


def _equal(got, want, ctx):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.size == w.size, (ctx, name, g.dtype, g.shape, w.shape)
        g = g.reshape(w.shape)
        bad = np.flatnonzero((g != w).reshape(len(w), -1).any(axis=1))[:5] if w.size else []
        assert not len(bad), (ctx, name, bad, g[bad], w[bad])


def _raw(kmc, kc, lo, hi, bases, offs, nc, spare=3):
    """kmc_correct through ctypes into arrays with `spare` entries more than needed, filled with a pattern"""
    L = kmc.lib()
    nr, nb = len(offs) - 1, len(bases)
    out, stats = np.full(nb + spare, 0xEE, U8), np.full(4 * nr + spare, 0xEEEEEEEE, U32)
    co, cands = np.full(nr + 1 + spare, 0xEEEE, U64), np.full(4 * (nc + spare), 0xEEEEEEEE, U32)
    n1 = C.c_uint64(12345)
    w = (C.c_uint64 * kmc.CORRECT_WORDS)()
    kc._chk(L.kmc_correct(kc._h, lo, hi, bases.ctypes.data, offs.ctypes.data, nr, out.ctypes.data, stats.ctypes.data, co.ctypes.data,
                          cands.ctypes.data, nc + spare, C.byref(n1), w))
    assert n1.value == nc
    assert (out[nb:] == 0xEE).all() and (stats[4 * nr:] == 0xEEEEEEEE).all() and (co[nr + 1:] == 0xEEEE).all() and (cands[4 * nc:] == 0xEEEEEEEE).all()
    return (out[:nb], stats[:4 * nr], co[:nr + 1], cands[:4 * nc]), list(w)


def _upload(bases, offs):
    import torch
    dev = torch.device("cuda", 0)
    db = torch.zeros(len(bases) + 64, dtype=torch.uint8, device=dev)
    db[:len(bases)] = torch.from_numpy(bases.copy())
    do = torch.from_numpy(offs.view(np.int64).copy()).to(dev)
    torch.cuda.synchronize(dev)
    return db, do


def _device(kc, lo, hi, bases, offs):
    """the device form on an uploaded batch, read back"""
    nr, nb = len(offs) - 1, len(bases)
    db, do = _upload(bases, offs)
    dc, ds, dco, dr, nc, s = kc.correct_reads_device(db.data_ptr(), do.data_ptr(), nr, nb, lo, hi)
    assert dc % 16 == 0 and ds % 16 == 0 and dco % 8 == 0 and dr % 16 == 0
    return (_dev_bytes(dc, nb), _dev_bytes(ds, 16 * nr).view(U32), _dev_u64(dco, nr + 1), _dev_bytes(dr, 16 * nc).view(U32)), nc, s.words()


def _check(kmc, kc, table, canonical, reads, ranges=RANGES):
    """every form of the call against the model, for every range; returns {range: the model's result}"""
    L = kmc.lib()
    bases, offs = ci.pack(reads)
    seen = {}
    for lo, hi in ranges:
        m = cm.correct_reads(table, canonical, reads, lo, hi, k=kc.k)
        want, words = _want(m), m.summary
        nc = words[4]
        ctx = (kc.k, canonical, lo, hi)
        # the sizing call
        n1 = C.c_uint64(1)
        w = (C.c_uint64 * 8)()
        kc._chk(L.kmc_correct(kc._h, lo, hi, bases.ctypes.data, offs.ctypes.data, len(reads), None, None, None, None, 0, C.byref(n1), w))
        assert (n1.value, list(w)) == (nc, words), (ctx, n1.value, list(w), words)
        got, w = _raw(kmc, kc, lo, hi, bases, offs, nc)
        assert w == words, (ctx, w, words)
        _equal(got, want, ctx + ("host",))
        got, dnc, w = _device(kc, lo, hi, bases, offs)
        assert (dnc, w) == (nc, words), (ctx, dnc, w, words)
        _equal(got, want, ctx + ("device",))
        r = kc.correct_reads(bases, offs, lo, hi)
        _equal((r.bases, r.stats, r.cand_offsets, r.cands), want, ctx + ("correct_reads",))
        assert r.summary.words() == words and len(r) == len(reads) and r.strings() == m.corrected
        assert list(r.fixes()) == m.fixes() and r.to_fasta() == m.text() and np.array_equal(r.offsets, offs)
        assert words[4] == int(r.cand_offsets[-1])
        seen[(lo, hi)] = m
    return seen


def _counter(kmc, oracle, sample, k, canonical):
    bases, offs = ci.pack(sample)
    want = oracle.count_kmers(bases, offs, k, canonical)
    table = _table_dict(want)
    assert table == gm.count_table(sample, k, canonical)
    kc = kmc.KmerCounter(k=k, canonical=canonical)
    kc.add_batch(bases, offs)
    assert kc.export().equals(want)
    return kc, table


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [5, 6, 31, 32, 33, 63])
def test_reads_corrected_and_gaps(kmc, oracle, k, canonical):
    """key widths and parities; both strands; N beside a weak run, lower case, reads of k - 1, k and k + 1 bases, empty reads,
    a read of N only; substituted reads counted in"""
    sample, reads = ci.genome_reads(k, 100 + k)
    kc, table = _counter(kmc, oracle, sample, k, canonical)
    with kc:
        seen = _check(kmc, kc, table, canonical, reads)
    if k >= 31:     # (at k = 5 and 6 the sample fills the k-mer space: those check exactness alone)
        w1, w2 = seen[(1, 0)].summary, seen[(2, 0)].summary
        assert w2[2] > w1[2] > 0 and w2[5] >= 40 and w2[3] > w2[4] > w2[5] and w1[5] >= 10, (w1, w2)
        assert {c[1] >> 16 & 255 for c in seen[(2, 0)].cands} == {0, 1, 2}


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [6, 31, 32, 63])
def test_placed_errors(kmc, oracle, k, canonical):
    """every place kmc.h tells apart, by name: the genome read counted twice, range (2, 0)"""
    sample, reads, names = ci.placed(k, 40 + k)
    kc, table = _counter(kmc, oracle, sample, k, canonical)
    bases, offs = ci.pack(reads)
    with kc:
        _check(kmc, kc, table, canonical, reads, ((2, 0),))
        r = kc.correct_reads(bases, offs, 2, 0)
    if k == 6:      # (a random read of 31 bases repeats 6-mers: exactness alone)
        return
    L = len(reads[0])
    got = lambda name: [(p, w >> 16 & 255, a, n, (w & 255) != (w >> 8 & 255))
                        for p, w, a, n in r.cands[int(r.cand_offsets[names[name]]):int(r.cand_offsets[names[name] + 1])].tolist()]
    assert got("clean") == []
    assert got("at_0") == [(0, kmc.CORRECT_HEAD, 0, 1, True)]
    assert got("at_k-1") == [(k - 1, kmc.CORRECT_HEAD, 0, k, True)]
    assert got("at_k") == [(k, kmc.CORRECT_INTERIOR, 1, k, True)]
    assert got("at_L-k-1") == [(L - k - 1, kmc.CORRECT_INTERIOR, L - 2 * k, k, True)]
    assert got("at_L-k") == [(L - k, kmc.CORRECT_TAIL, L - 2 * k + 1, k, True)]
    assert got("at_L-1") == [(L - 1, kmc.CORRECT_TAIL, L - k, 1, True)]
    assert got("two_k+1_apart") == [(k, kmc.CORRECT_INTERIOR, 1, k, True), (2 * k + 1, kmc.CORRECT_INTERIOR, k + 2, k, True)]
    for name in ("two_k_apart", "two_k-1_apart", "before_N", "weak_end_to_end"):
        assert got(name) == [] and r.strings()[names[name]] == reads[names[name]], name
    assert r.stats[names["two_k_apart"]].tolist() == [L - k + 1, 2 * k, 0, 0]
    assert r.stats[names["two_k-1_apart"]].tolist() == [L - k + 1, 2 * k - 1, 0, 0]
    assert r.stats[names["weak_end_to_end"]].tolist() == [k, k, 0, 0]
    for name in ("at_0", "at_k-1", "at_k", "at_L-k-1", "at_L-k", "at_L-1", "two_k+1_apart"):
        assert r.strings()[names[name]] == reads[0], name


@pytest.mark.parametrize("canonical", [True, False])
def test_ambiguity_and_the_range(kmc, oracle, canonical):
    k = 31
    sample, reads, p, ref, alt = ci.snp(k, 11)
    kc, table = _counter(kmc, oracle, sample, k, canonical)
    bases, offs = ci.pack(reads)
    with kc:
        _check(kmc, kc, table, canonical, reads, ((2, 0), (3, 0)))
        r = kc.correct_reads(bases, offs, 2, 0)
        (q, word, a, n), = r.cands[:int(r.cand_offsets[1])].tolist()
        assert q == p and word >> 24 == (1 << "ACGT".index(ref) | 1 << "ACGT".index(alt)) and (word & 255) == (word >> 8 & 255) == ord(reads[0][p])
        assert r.strings() == reads and r.summary.ambiguous == 1 and r.summary.corrected == 0
        r = kc.correct_reads(bases, offs, 3, 0)
        assert r.strings()[0] == reads[1] and list(r.fixes())[0] == (0, p, reads[0][p], ref, kmc.CORRECT_INTERIOR)


@pytest.mark.parametrize("canonical", [True, False])
def test_runs_across_chunk_edges_and_a_waves_span(kmc, oracle, canonical):
    k = 31
    sample, reads = ci.seams(k, 7)
    kc, table = _counter(kmc, oracle, sample, k, canonical)
    with kc:
        m = _check(kmc, kc, table, canonical, reads, ((2, 0),))[(2, 0)]
    assert m.stats[0] == [2970, 6 * k, 6, 6] and m.corrected[0] == sample[0] and m.summary[5] == 8
    sample, reads = ci.starts_at_1024(k, 8)
    assert len(reads[0]) == 1024
    kc, table = _counter(kmc, oracle, sample, k, canonical)
    with kc:
        m = _check(kmc, kc, table, canonical, reads, ((2, 0),))[(2, 0)]
    assert [s[3] for s in m.stats] == [1, 1, 1, 1] and [c[1] >> 16 & 255 for c in m.cands] == [2, 1, 0, 2]


@pytest.mark.parametrize("canonical", [True, False])
def test_candidates_on_both_sides_of_every_tile_edge(kmc, oracle, canonical):
    k = 31
    sample, reads = ci.many_short(k, 10)
    kc, table = _counter(kmc, oracle, sample, k, canonical)
    with kc:
        m = _check(kmc, kc, table, canonical, reads, ((2, 0),))[(2, 0)]
    assert len(reads) == 3000 and m.summary[4] >= 2900 and m.summary[5] >= 2900 and sum(len(r) for r in reads) > 80 * 2048


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [31, 32])
def test_round_trip_on_the_device(kmc, oracle, k, canonical):
    """the corrected device array and the caller's offsets go into add_batch_device of a second ctx; correcting the corrected
    batch again corrects nothing"""
    sample, reads = ci.genome_reads(k, 300 + k)
    kc, table = _counter(kmc, oracle, sample, k, canonical)
    m = cm.correct_reads(table, canonical, reads, 2, 0)
    bases, offs = ci.pack(reads)
    cb, co = ci.pack(m.corrected)
    want = oracle.count_kmers(cb, co, k, canonical)
    with kc, kmc.KmerCounter(k=k, canonical=canonical) as second:
        db, do = _upload(bases, offs)
        dc, _, _, _, nc, s = kc.correct_reads_device(db.data_ptr(), do.data_ptr(), len(reads), len(bases), 2, 0)
        assert s.words() == m.summary and nc == m.summary[4]
        second.add_batch_device(dc, do.data_ptr(), len(reads), len(bases), 0)
        assert second.export().equals(want)
        first = kc.correct_reads(bases, offs, 2, 0)
        again = kc.correct_reads(first.bases, offs, 2, 0)
        assert again.summary.corrected == 0 and again.summary.weak_windows == first.summary.weak_windows_left
        assert np.array_equal(again.bases, first.bases) and first.summary.corrected >= 40


_CHILD = r"""
import importlib, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
kmc = importlib.import_module("k-mer-count_amd")
bases, offs = kmc.parse_fasta(sys.argv[2])
same = lambda a, b: all(np.array_equal(getattr(a, f), getattr(b, f)) for f in sys.argv[3].split(","))
with kmc.KmerCounter(k=31) as kc:
    kc.add_batch(bases, offs)
    kc.finalize()
    print("step first", file=sys.stderr, flush=True)
    u = kc.unitigs(1, 0)
    l = kc.unitig_links(1, 0)
    v = kc.clean_unitigs(1, 0)
    a = kc.map_reads(bases, offs, 1, 0)
    print("step correct", file=sys.stderr, flush=True)
    c1 = kc.correct_reads(bases, offs, 2, 0)
    print("step again", file=sys.stderr, flush=True)
    u2 = kc.unitigs(1, 0)
    kc.correct_reads(bases, offs, 1, 0)
    l2 = kc.unitig_links(1, 0)
    kc.correct_reads(bases, offs, 2, 3)
    v2 = kc.clean_unitigs(1, 0)
    kc.correct_reads(bases, offs, 2, 0)
    b = kc.map_reads(bases, offs, 1, 0)
    print("step end", file=sys.stderr, flush=True)
    assert np.array_equal(u.bases, u2.bases) and np.array_equal(u.offsets, u2.offsets) and np.array_equal(u.abund, u2.abund)
    assert np.array_equal(l.to, l2.to) and np.array_equal(l.offsets, l2.offsets) and np.array_equal(v.verdict, v2.verdict)
    assert same(a, b)
    c2 = kc.correct_reads(bases, offs, 2, 0)
    assert np.array_equal(c1.bases, c2.bases) and np.array_equal(c1.cands, c2.cands)
"""


def test_correct_leaves_the_other_results_alone(kmc):
    """What computes, seen through the KMC_UNITIG_TRACE lines of a child process (nothing is timed): correct calls between
    unitigs, links, clean and map of one range make none of them compute again"""
    env = dict(os.environ, KMC_UNITIG_TRACE="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, SAMPLE, "place,stats,seg_offsets,segments,support"], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    steps, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("step "):
            cur = line[5:]
            steps[cur] = []
        elif line.startswith("kmc_"):
            steps[cur].append(line.split(":")[0] + (" reused" if "unitigs_reused 1" in line else ""))
    assert steps["first"][0] == "kmc_unitigs" and steps["first"].count("kmc_unitigs") == 1
    assert steps["correct"] == ["kmc_correct"]
    # unitigs, links and the clean pass copy from what the ctx holds; the map call computes on every call, on the unitigs kept
    assert steps["again"] == ["kmc_correct", "kmc_correct", "kmc_correct", "kmc_unitig_map reused"], steps["again"]
    assert "mark_ms" in r.stderr and "runs_ms" in r.stderr and "try_ms" in r.stderr


def test_empty_inputs_and_errors(kmc, oracle):
    L = kmc.lib()
    k = 31
    sample, reads = ci.genome_reads(k, 5, n_reads=40, genome=600)
    bases, offs = ci.pack(reads)
    w = (C.c_uint64 * 8)(*([7] * 8))
    n1 = C.c_uint64(9)
    args = lambda b, o, n: (b.ctypes.data, o.ctypes.data, n, None, None, None, None, 0, C.byref(n1), w)
    with kmc.KmerCounter(k=k) as kc:
        # no view
        assert L.kmc_correct(kc._h, 1, 0, *args(bases, offs, len(reads))) == kmc.ERR_STATE
        assert L.kmc_correct_device(kc._h, 1, 0, None, None, 0, 0, None, None, None, None, None, None) == kmc.ERR_STATE
        # an empty view: no candidate, the batch back as it came, its valid windows all weak and counted
        kc.finalize()
        m = cm.correct_reads({}, True, reads, 1, 0, k=k)
        r = kc.correct_reads(bases, offs, 1, 0)
        assert r.summary.words() == m.summary and m.summary[1] == m.summary[2] == m.summary[7] > 0 and m.summary[4] == 0
        assert np.array_equal(r.bases, bases) and len(r.cands) == 0 and not r.cand_offsets.any()
        assert np.array_equal(r.stats, np.array(m.stats, U32))
    kc, table = _counter(kmc, oracle, sample, k, True)
    with kc:
        # n_reads == 0
        z = np.zeros(1, U64)
        r = kc.correct_reads(np.zeros(0, U8), z)
        assert r.summary.words() == [0] * 8 and len(r.bases) == 0 and list(r.cand_offsets) == [0] and len(r.cands) == 0
        assert L.kmc_correct(kc._h, 1, 0, None, None, 0, None, None, None, None, 0, C.byref(n1), w) == 0
        assert (n1.value, list(w)) == (0, [0] * 8)
        # arguments
        assert L.kmc_correct(None, 1, 0, *args(bases, offs, len(reads))) == kmc.ERR_ARG
        assert L.kmc_correct(kc._h, 3, 2, *args(bases, offs, len(reads))) == kmc.ERR_ARG
        bad = offs.copy()
        bad[3] = bad[2] - 1
        assert L.kmc_correct(kc._h, 1, 0, *args(bases, bad, len(reads))) == kmc.ERR_ARG
        # a cap one too small: KMC_ERR_ARG, the count is set and nothing is written
        m = cm.correct_reads(table, True, reads, 2, 0)
        nc = m.summary[4]
        assert nc > 1
        cands, out, co = np.full(4 * nc, 0xEEEEEEEE, U32), np.full(len(bases), 0xEE, U8), np.full(len(offs), 0xEEEE, U64)
        rc = L.kmc_correct(kc._h, 2, 0, bases.ctypes.data, offs.ctypes.data, len(reads), out.ctypes.data, None, co.ctypes.data, cands.ctypes.data,
                           nc - 1, C.byref(n1), None)
        assert rc == kmc.ERR_ARG and n1.value == nc
        assert (cands == 0xEEEEEEEE).all() and (out == 0xEE).all() and (co == 0xEEEE).all()
        # ... and an array that is NULL has no cap
        assert L.kmc_correct(kc._h, 2, 0, bases.ctypes.data, offs.ctypes.data, len(reads), out.ctypes.data, None, None, None, 0, C.byref(n1), None) == 0
        assert n1.value == nc and out.tobytes().decode() == "".join(m.corrected)
    with kmc.KmerCounter(mode=kmc.MODE_LR) as lr:
        assert L.kmc_correct(lr._h, 1, 0, *args(bases, offs, len(reads))) == kmc.ERR_ARG
        assert L.kmc_correct_device(lr._h, 1, 0, None, None, 0, 0, None, None, None, None, None, None) == kmc.ERR_ARG


def _sample_reads(kmc):
    bases, offs = kmc.parse_fasta(SAMPLE)
    return [bases[int(offs[i]):int(offs[i + 1])].tobytes().decode() for i in range(len(offs) - 1)]


@pytest.mark.parametrize("forward", [False, True])
def test_cli_correct(kmc, forward):
    k, canonical = 31, not forward
    reads = _sample_reads(kmc)
    table = gm.count_table(reads, k, canonical)
    fw = ["--forward"] if forward else []
    run = lambda *a: subprocess.run([EXE, SAMPLE, "-k", str(k), "--correct", SAMPLE] + list(a) + fw, capture_output=True, text=True)
    r = run()
    assert r.returncode == 0 and r.stdout == cm.correct_reads(table, canonical, reads).text(), r.stderr
    r = run("--min-count", "2")
    assert r.returncode == 0 and r.stdout == cm.correct_reads(table, canonical, reads, 2, 0).text(), r.stderr
    if not forward:
        final = bm.rounds(table, canonical, max_bubble=31, n_rounds=1)[0]
        r = run("--clean", "1", "--bubble-keys", "31")
        assert r.returncode == 0 and r.stdout == cm.correct_reads(final, canonical, reads, k=k).text(), r.stderr
    for bad in (["--map", SAMPLE], ["--profile", SAMPLE], ["--graph"], ["--histo", "5"]):
        assert run(*bad).returncode == 2
    assert subprocess.run([EXE, SAMPLE, "--correct", SAMPLE], capture_output=True).returncode == 2      # needs -k
