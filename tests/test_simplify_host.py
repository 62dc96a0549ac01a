"""CPU-side checks of bubble popping: the three kmc_unitig_simplify* entry points are exported and keep their argument rules
without a device, the header section, the CLI knows --bubble-keys and rejects it without --clean before touching a GPU,
SimplifySummary, and the model the GPU tests compare against (tests/bubble_model.py): the substitution bubble with its
known answer, every hand-built input of bubble_inputs.py, the model against its numpy restatement, the equivalence to
clean_model with the bubble limit 0, and the property that of two parallel arms at most one is popped."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bubble_inputs as bi
import bubble_model as bm
import clean_inputs as ci
import clean_model as cm
import graph_model as gm
import links_model as lm
import unitig_model as um
from conftest import ROOT, SAMPLE
from test_clean_host import model_objects
from test_unitig_host import _random_reads

NEW = ("kmc_unitig_simplify", "kmc_unitig_simplify_device", "kmc_unitig_simplify_into")
EXE = os.path.join(ROOT, "bin", "k-mer-count")
BIG = 1 << 31


def test_library_exports_the_simplify_calls(kmc):
    out = subprocess.run(["nm", "-D", "--defined-only", kmc.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for s in NEW:
        assert f" T {s}\n" in out, s
        assert s in kmc.ABI_SYMBOLS
    L = kmc.lib()
    vp, u64, pu64 = C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)
    assert L.kmc_unitig_simplify_device.argtypes == [vp, u64, u64, u64, u64, u64] + [C.POINTER(vp)] * 4 + [pu64, pu64, vp]
    assert L.kmc_unitig_simplify.argtypes == [vp, u64, u64, u64, u64, u64, vp, vp, vp, u64, vp, u64, pu64, pu64, vp]
    assert L.kmc_unitig_simplify_into.argtypes == [vp, vp, u64, u64, u64, u64, u64, vp]
    a = np.full(12, 7, np.uint64)
    p = a.ctypes.data
    n1, n2 = C.c_uint64(7), C.c_uint64(7)
    # a NULL ctx: KMC_ERR_ARG, the sizes zeroed, nothing written
    assert L.kmc_unitig_simplify(None, 1, 0, 5, 5, 5, p, p, p, 4, p, 4, C.byref(n1), C.byref(n2), p) == kmc.ERR_ARG
    assert n1.value == 0 and n2.value == 0 and (a == 7).all()
    assert L.kmc_unitig_simplify(None, 1, 0, 5, 5, 5, None, None, None, 0, None, 0, None, None, None) == kmc.ERR_ARG
    assert L.kmc_unitig_simplify_device(None, 1, 0, 5, 5, 5, None, None, None, None, None, None, None) == kmc.ERR_ARG
    assert L.kmc_unitig_simplify_into(None, None, 1, 0, 5, 5, 5, None) == kmc.ERR_ARG
    assert kmc.SIMPLIFY_WORDS == 12 == len(bm.FIELDS) and kmc.CLEAN_WORDS == 8
    assert kmc.CLEAN_BUBBLE == bm.BUBBLE == 3


def test_header_declares_the_simplify_section():
    hdr = open(os.path.join(ROOT, "include", "kmc.h")).read()
    assert "#define KMC_SIMPLIFY_WORDS 12" in hdr and "#define KMC_CLEAN_BUBBLE 3" in hdr and "#define KMC_CLEAN_WORDS 8" in hdr
    for phrase in ("BUBBLE CANDIDATE.", "PARALLEL.", "A simplify call counts as a clean call", "NOT added to the surviving arm",
                   "kmc_unitig_simplify: keys N unitigs U tips T islands I bubbles B kept K"):
        assert phrase in " ".join(hdr.replace(" * ", " ").split()), phrase
    assert "kmc_unitig_simplify / kmc_unitig_simplify_device / kmc_unitig_simplify_into" in hdr.split("Conventions")[0]


@pytest.mark.parametrize("argv", [
    ["-k", "5", "--bubble-keys", "3"],                                                   # without --clean
    ["-k", "5", "--clean", "1", "--bubble-keys", "-1"], ["-k", "5", "--clean", "1", "--bubble-keys", "x"],
    ["-k", "5", "--clean", "1", "--bubble-keys"]])
def test_cli_rejects_bad_bubble_options(kmc, argv):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")   # no GPU to touch even where there is one
    r = subprocess.run([EXE, SAMPLE] + argv, capture_output=True, text=True, env=env)
    assert r.returncode == 2 and r.stdout == "" and "k-mer-count:" in r.stderr, (argv, r.returncode, r.stderr)
    assert "unknown option" not in r.stderr, r.stderr


def test_cli_help_lists_bubble_keys(kmc):
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == ""
    assert "--clean ROUNDS [--tip-keys N] [--island-keys N] [--bubble-keys N]" in r.stderr


def test_simplify_summary_object(kmc):
    w = [16, 6, 1, 300, 30, 3, 9, 4000, 2, 62, 5, 70]
    s = kmc.SimplifySummary.from_words(np.array(w, np.uint64))
    assert s.words() == w and all(type(x) is int for x in s.words())
    assert (s.bubbles, s.bubble_keys, s.bubble_candidates, s.bubble_count) == (2, 62, 5, 70)
    assert (s.unitigs, s.tips, s.islands, s.kept_keys, s.tip_keys, s.island_keys, s.tip_candidates, s.kept_count) == tuple(w[:8])
    assert s.removed == 9
    assert s.to_text() == "".join("%s\t%d\n" % (f, v) for f, v in zip(bm.FIELDS, w))
    assert kmc.CleanSummary.from_words(w[:8]).removed == 7                   # the clean summary is as it was


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [5, 21, 31, 32, 63])
def test_the_substitution_bubble(k, canonical):
    reads, s, err = bi.substitution(k, 10 + k)
    table = gm.count_table(reads, k, canonical)
    assert len(table) == 6 * k + 1
    old = cm.clean(table, canonical)
    assert old.verdict == [cm.KEEP] * 4 and old.kept == table                 # neither a tip nor an island: clean keeps it
    c = bm.simplify(table, canonical)
    u = c.unitigs
    m = [len(x) - k + 1 for x in u.seqs]
    assert sorted(zip(m, u.abund)) == sorted([(2 * k, 6 * k), (2 * k + 1, 6 * k + 3), (k, 3 * k), (k, k)])
    arm = bi.unitig_with(u, err[:k], k, canonical)
    true_arm = bi.unitig_with(u, s[2 * k + 1:3 * k + 1], k, canonical)
    assert arm != true_arm and (m[arm], u.abund[arm], m[true_arm], u.abund[true_arm]) == (k, k, k, 3 * k)
    assert c.verdict == [bm.BUBBLE if i == arm else bm.KEEP for i in range(4)]
    assert sorted(c.bubble_candidates) == sorted([arm, true_arm])
    assert c.summary == [4, 0, 0, 5 * k + 1, 0, 0, 0, 3 * (5 * k + 1), 1, k, 2, k]
    assert c.kept == gm.count_table([s] * 3, k, canonical)
    final, words = bm.rounds(table, canonical, n_rounds=4)
    assert len(words) == 2 and words[1] == [1, 0, 0, 5 * k + 1, 0, 0, 0, 3 * (5 * k + 1), 0, 0, 0, 0] and final == c.kept
    assert [len(x) - k + 1 for x in um.unitigs(final, canonical).seqs] == [5 * k + 1]
    # the bubble limit just below the arm: nothing is a candidate
    assert bm.simplify(table, canonical, max_bubble=k - 1).summary[8:] == [0, 0, 0, 0]
    # the tip and island rounds alone never get rid of it
    assert cm.rounds(table, canonical, n_rounds=4)[0] == table


def _inputs(k, canonical):
    """(name, table) of every builder of bubble_inputs"""
    t = lambda reads: gm.count_table(reads, k, canonical)
    return [("substitution", t(bi.substitution(k, 10 + k)[0])), ("three_arms", t(bi.three_arms(k, 20 + k)[0])),
            ("k_and_k_plus_1", t(bi.arms_k_and_k_plus_1(k, 30 + k)[0])), ("decided_pairs", t(bi.decided_pairs(k, 40 + k)[0])),
            ("wide", bi.wide_bubble(k, canonical, 50 + k)[0]), ("tip_and_bubble", t(bi.tip_and_bubble(k, 60 + k)[0])),
            ("circular", t([bi.circular(k, 70 + k)] + bi.substitution(k, 10 + k)[0])), ("same_end", t(bi.same_end(k, 80 + k)[0])),
            ("everything", t(bi.everything(k, 90 + k))), ("field", t(bi.field(k, 100 + k)[0])),
            ("clean_forks", t(ci.five_forks(k, 100 + k)[0] + ci.islands(k, 200 + k) + ci.rounds_input(k, 400 + k)))]


def _ends(lk, u):
    r0, r1 = (lk.to[lk.offsets[e]:lk.offsets[e + 1]] for e in (2 * u, 2 * u + 1))
    return frozenset((r0[0], r1[0])) if len(r0) == 1 and len(r1) == 1 else None


def _no_two_parallel_arms_popped(c, ctx):
    """The order is strict: of two parallel arms never both are popped for one another's sake.  Said for classes of any
    size (three arms between the same two ends lose two, the three_arms input): no class of parallel candidates is popped
    whole, so a class of two loses at most one and the two junctions stay connected."""
    popped = [u for u, v in enumerate(c.verdict) if v == bm.BUBBLE]
    assert set(popped) <= set(c.bubble_candidates) and not set(c.bubble_candidates) & set(c.candidates), ctx
    classes = {}
    for u in c.bubble_candidates:
        e = _ends(c.links, u)
        assert e is not None and len(e) == 2, ctx
        classes.setdefault(e, []).append(u)
    for e, arms in classes.items():
        gone = [u for u in arms if c.verdict[u] == bm.BUBBLE]
        assert len(gone) < len(arms), (ctx, arms)
        assert len(arms) > 1 or not gone, (ctx, arms)


def _against_numpy(kmc, table, canonical, c, limits, ctx):
    k = len(next(iter(table)))
    t, uo, lo = model_objects(kmc, table, canonical, c)
    if k <= 31:
        key_lo, cnt, verdict, words = bm.np_simplify(t, uo, lo, k, canonical, *limits)
        keys = sorted(c.kept)
        assert words == c.summary, (ctx, words, c.summary)
        assert [int(x) for x in key_lo] == [kmc.encode_key(x, False)[1] for x in keys] and [int(x) for x in cnt] == [c.kept[x] for x in keys], ctx
    else:
        verdict, bcand = bm.np_verdicts(uo.offsets, uo.abund, uo.flags, lo.offsets, lo.to, k, *limits)
        assert sorted(np.flatnonzero(bcand)) == sorted(c.bubble_candidates), ctx
    assert list(verdict) == c.verdict, ctx


def _triples(k):
    return ((k, k, k), (0, 0, 0), (0, 0, k), (k, k, 0), (BIG, BIG, BIG), (1, 1, 1), (k, k, k + 1))


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [5, 21, 32, 63])
def test_model_and_numpy_on_the_built_inputs(kmc, k, canonical):
    levels = {"abundance": 0, "keys": 0, "id": 0}
    seen = {}
    for name, table in _inputs(k, canonical):
        graph = (um.unitigs(table, canonical), lm.links(table, canonical))
        for limits in _triples(k):
            ctx = (name, k, canonical, limits)
            c = bm.simplify(table, canonical, 1, 0, *limits, graph=graph)
            w = c.summary
            assert w[3] + w[4] + w[5] + w[9] == graph[0].summary[2] and w[8] <= w[10] and w[7] + w[11] <= sum(table.values()), ctx
            assert all(c.verdict[u] == bm.KEEP for u, f in enumerate(c.unitigs.flags) if f), ctx
            _no_two_parallel_arms_popped(c, ctx)
            _against_numpy(kmc, table, canonical, c, limits, ctx)
            if limits[2] == 0:
                old = cm.clean(table, canonical, 1, 0, limits[0], limits[1], graph=graph)
                assert (c.verdict, c.kept, w[:8], w[8:]) == (old.verdict, old.kept, old.summary, [0] * 4), ctx
            for l in levels:
                levels[l] += c.bubble_levels[l]
            seen[(name, limits)] = c
    if k < 21:
        return                                                               # (at k = 5 the random sequences branch on their own)
    assert all(levels.values()), levels                                      # every level of the comparison decided somewhere
    kk = (k, k, k)
    assert seen[("three_arms", kk)].summary[8:11] == [2, 2 * k, 3]
    assert seen[("k_and_k_plus_1", kk)].summary[8:11] == [1, k, 2] and seen[("k_and_k_plus_1", (k, k, k + 1))].summary[8:11] == [2, 2 * k + 1, 4]
    assert seen[("decided_pairs", kk)].summary[8:11] == [3, 3 * k - 1, 6]
    assert seen[("decided_pairs", kk)].bubble_levels == {"abundance": 2, "keys": 2, "id": 2}
    assert seen[("tip_and_bubble", kk)].summary[:3] == [5, 1, 0] and seen[("tip_and_bubble", kk)].summary[8:11] == [1, k, 2]
    assert seen[("tip_and_bubble", (0, 0, k))].summary[1] == 0 and seen[("tip_and_bubble", (k, k, 0))].summary[8] == 0
    assert seen[("circular", kk)].summary[8] == 1 and sum(seen[("circular", kk)].unitigs.flags) == 1
    assert seen[("field", kk)].summary[8:11] == [320, 320 * k, 640] and seen[("field", kk)].summary[0] == 1280
    c = seen[("same_end", (BIG, BIG, BIG))]
    if canonical:                                                            # one unitig whose two ends reach the same end
        loop = [u for u in range(len(c.verdict)) if _ends(c.links, u) is not None]
        assert len(loop) == 1 and len(_ends(c.links, loop[0])) == 1 and c.bubble_candidates == [] and c.verdict[loop[0]] == bm.KEEP


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [21, 32, 33])
def test_model_compares_wide_products(k, canonical):
    table, true_arm, ins_arm = bi.wide_bubble(k, canonical, 50 + k)
    c = bm.simplify(table, canonical)
    ut, ui = bi.unitig_with(c.unitigs, true_arm[0], k, canonical), bi.unitig_with(c.unitigs, ins_arm[0], k, canonical)
    at, ai = c.unitigs.abund[ut], c.unitigs.abund[ui]
    assert (at, ai) == (((1 << 64) - 1) // k, -(-(1 << 64) // (k - 1)) + 7)
    assert (c.verdict[ut], c.verdict[ui]) == (bm.BUBBLE, bm.KEEP) and c.bubble_levels["abundance"] == 2
    # what a 64-bit product would have decided
    assert (ai * (k - 1)) % (1 << 64) < (at * k) % (1 << 64)
    assert c.summary[11] == at and c.summary[7] + c.summary[11] == sum(table.values()) < 1 << 64


def _mutated_reads(rng, k, n, times):
    """a random sequence of n bases read twice and `times` stretches of it with one base changed: bubbles among whatever
    else a small k makes of it"""
    s = ci.rnd(rng, n)
    reads = [s, s]
    for _ in range(times):
        p = int(rng.integers(k, len(s) - k))
        alt = "ACGT"[("ACGT".index(s[p]) + 1 + int(rng.integers(0, 3))) % 4]
        reads.append(s[max(p - k - 2, 0):p] + alt + s[p + 1:p + k + 3])
    return reads


@pytest.mark.parametrize("k", [2, 3, 4, 5, 6, 7, 8])
def test_no_two_parallel_arms_are_popped_on_random_reads(kmc, k):
    """small random tables branch everywhere; even k in a canonical ctx has palindromic keys, dropped and one-sided records.
    Every other table is dense (the reads of the unitig tests and a mutated sequence of 80 bases), the others are 30 bases
    with three mutations, where a k of 5 still leaves bubbles standing."""
    rng = np.random.default_rng(6000 + k)
    popped = 0
    for canonical in (True, False):
        for trial in range(8):
            reads = _mutated_reads(rng, k, 30, 3) if trial % 2 else _random_reads(rng, k) + _mutated_reads(rng, k, 80, 12)
            table = gm.count_table(reads, k, canonical)
            for lo, hi in ((1, 0), (2, 0), (1, 1)):
                graph = (um.unitigs(table, canonical, lo, hi), lm.links(table, canonical, lo, hi))
                for limits in ((k, k, k), (3 * k, 3 * k, 3 * k), (0, 0, BIG), (1, 1, 1), (BIG, BIG, BIG)):
                    ctx = (k, canonical, trial, lo, hi, limits)
                    c = bm.simplify(table, canonical, lo, hi, *limits, graph=graph)
                    w = c.summary
                    assert w[0] == graph[0].summary[0] and w[3] + w[4] + w[5] + w[9] == graph[0].summary[2], ctx
                    assert w[3] == len(c.kept) and w[7] == sum(c.kept.values()), ctx
                    _no_two_parallel_arms_popped(c, ctx)
                    old = cm.clean(table, canonical, lo, hi, limits[0], limits[1], graph=graph)
                    assert [v if v != bm.BUBBLE else bm.KEEP for v in c.verdict] == old.verdict and w[:3] == old.summary[:3], ctx
                    if (lo, hi) == (1, 0) and trial < 4:
                        _against_numpy(kmc, table, canonical, c, limits, ctx)
                    popped += w[8]
    if k >= 5:
        assert popped > 0


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [5, 15, 31, 32])
def test_model_and_numpy_on_sample_fasta(kmc, k, canonical):
    bases, offs = kmc.parse_fasta(SAMPLE)
    text = bytes(bases).decode()
    reads = [text[int(offs[i]):int(offs[i + 1])] for i in range(len(offs) - 1)]
    table = gm.count_table(reads, k, canonical)
    for lo, hi in ((1, 0), (2, 0)):
        graph = (um.unitigs(table, canonical, lo, hi), lm.links(table, canonical, lo, hi))
        for limits in ((k, k, k), (0, 0, k), (BIG, BIG, BIG)):
            c = bm.simplify(table, canonical, lo, hi, *limits, graph=graph)
            _no_two_parallel_arms_popped(c, (k, canonical, lo, hi, limits))
            if (lo, hi) == (1, 0):                 # (the numpy route looks its keys up in the whole table: every key solid)
                _against_numpy(kmc, table, canonical, c, limits, (k, canonical, limits))
            else:
                t, uo, lk = model_objects(kmc, table, canonical, c)
                v, bc = bm.np_verdicts(uo.offsets, uo.abund, uo.flags, lk.offsets, lk.to, k, *limits)
                assert list(v) == c.verdict and sorted(np.flatnonzero(bc)) == sorted(c.bubble_candidates)
