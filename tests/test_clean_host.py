"""CPU-side checks of the graph cleaning: the three entry points are exported and keep their argument rules without a device,
the header section, the CLI knows --clean and rejects bad uses of it before touching a GPU, CleanSummary, and the Python
model the GPU tests compare against (tests/clean_model.py): hand-built forks and islands with known answers, a decision that
needs a 128-bit product, the rounds loop, the summary identity, and verdicts recomputed from links that were found by
brute force over the spelled unitig strings."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import clean_inputs as ci
import clean_model as cm
import graph_model as gm
import links_model as lm
import unitig_model as um
from conftest import ROOT, SAMPLE
from test_unitig_host import _random_reads

NEW = ("kmc_unitig_clean", "kmc_unitig_clean_device", "kmc_unitig_clean_into")
EXE = os.path.join(ROOT, "bin", "k-mer-count")
KS = [21, 32, 33]


def test_library_exports_the_clean_calls(kmc):
    out = subprocess.run(["nm", "-D", "--defined-only", kmc.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for s in NEW:
        assert f" T {s}\n" in out, s
        assert s in kmc.ABI_SYMBOLS
    L = kmc.lib()
    vp, u64, pu64 = C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)
    assert L.kmc_unitig_clean_device.argtypes == [vp, u64, u64, u64, u64] + [C.POINTER(vp)] * 4 + [pu64, pu64, vp]
    assert L.kmc_unitig_clean.argtypes == [vp, u64, u64, u64, u64, vp, vp, vp, u64, vp, u64, pu64, pu64, vp]
    assert L.kmc_unitig_clean_into.argtypes == [vp, vp, u64, u64, u64, u64, vp]
    a = np.full(8, 7, np.uint64)
    p = a.ctypes.data
    n1, n2 = C.c_uint64(7), C.c_uint64(7)
    # a NULL ctx: KMC_ERR_ARG, the sizes zeroed, nothing written
    assert L.kmc_unitig_clean(None, 1, 0, 5, 5, p, p, p, 4, p, 4, C.byref(n1), C.byref(n2), p) == kmc.ERR_ARG
    assert n1.value == 0 and n2.value == 0 and (a == 7).all()
    assert L.kmc_unitig_clean(None, 1, 0, 5, 5, None, None, None, 0, None, 0, None, None, None) == kmc.ERR_ARG
    assert L.kmc_unitig_clean_device(None, 1, 0, 5, 5, None, None, None, None, None, None, None) == kmc.ERR_ARG
    assert L.kmc_unitig_clean_into(None, None, 1, 0, 5, 5, None) == kmc.ERR_ARG
    assert kmc.CLEAN_WORDS == 8 == len(cm.FIELDS)
    assert (kmc.CLEAN_KEEP, kmc.CLEAN_TIP, kmc.CLEAN_ISLAND) == (cm.KEEP, cm.TIP, cm.ISLAND) == (0, 1, 2)


def test_header_declares_the_clean_section():
    hdr = open(os.path.join(ROOT, "include", "kmc.h")).read()
    assert "#define KMC_CLEAN_WORDS 8" in hdr
    for name, v in (("KEEP", 0), ("TIP", 1), ("ISLAND", 2)):
        assert "#define KMC_CLEAN_%s %d" % (name, v) in hdr
    assert "A clean call counts as a kmc_unitig_links* call" in hdr and "128-bit products" in hdr
    assert "kmc_unitig_clean / kmc_unitig_clean_device / kmc_unitig_clean_into" in hdr.split("Conventions")[0]   # the mapping table at the top


@pytest.mark.parametrize("argv", [
    ["--clean", "1"],                                                                    # without -k
    ["-k", "5", "--tip-keys", "3"], ["-k", "5", "--island-keys", "3"],                   # without --clean
    ["-k", "5", "--clean", "0"], ["-k", "5", "--clean", "x"], ["-k", "5", "--clean"], ["-k", "5", "--clean", "1", "--tip-keys", "-1"],
    ["-k", "5", "--clean", "1", "--with", "SAMPLE", "--compare"], ["-k", "5", "--clean", "1", "--with", "SAMPLE", "--setop", "union"],
    ["-k", "5", "--clean", "1", "--with", "SAMPLE"],
    ["-k", "5", "--clean", "1", "--min-count", "3", "--max-count", "2"]])
def test_cli_rejects_bad_clean_options(kmc, argv):
    argv = [SAMPLE if a == "SAMPLE" else a for a in argv]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")   # no GPU to touch even where there is one
    r = subprocess.run([EXE, SAMPLE] + argv, capture_output=True, text=True, env=env)
    assert r.returncode == 2 and r.stdout == "" and "k-mer-count:" in r.stderr, (argv, r.returncode, r.stderr)
    assert "unknown option" not in r.stderr, r.stderr


def test_cli_help_lists_clean(kmc):
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == ""
    assert "--clean ROUNDS [--tip-keys N] [--island-keys N]" in r.stderr


def test_clean_summary_object(kmc):
    w = [16, 6, 1, 300, 30, 3, 9, 4000]
    s = kmc.CleanSummary.from_words(np.array(w, np.uint64))
    assert s.words() == w and all(type(x) is int for x in s.words())
    assert (s.unitigs, s.tips, s.islands, s.kept_keys, s.tip_keys, s.island_keys, s.tip_candidates, s.kept_count) == tuple(w)
    assert s.removed == 7
    assert s.to_text() == "".join("%s\t%d\n" % (f, v) for f, v in zip(cm.FIELDS, w))


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", KS)
def test_model_on_the_five_forks(k, canonical):
    reads, arms = ci.five_forks(k, 100 + k)
    table = gm.count_table(reads, k, canonical)
    c = cm.clean(table, canonical)             # limits (k, k)
    u = c.unitigs
    assert c.summary[0] == 16 and c.summary[6] == 9 and c.summary[1] == 6 and c.summary[2] == 0, c.summary
    ids = [[ci.unitig_of(u, a, k, canonical) for a in f] for f in arms]
    keys = lambda i: len(u.seqs[i]) - k + 1
    v = c.verdict
    # fork 1: the once-seen arm goes, the twice-seen stays
    assert (v[ids[0][0]], v[ids[0][1]]) == (cm.KEEP, cm.TIP) and u.abund[ids[0][0]] == 2 * u.abund[ids[0][1]] == 10
    # fork 2: equal means, the 5-key arm goes, the 7-key arm stays
    assert (keys(ids[1][0]), keys(ids[1][1])) == (5, 7) and (v[ids[1][0]], v[ids[1][1]]) == (cm.TIP, cm.KEEP)
    # fork 3: equal in everything: the larger id goes
    lo, hi = sorted(ids[2])
    assert keys(lo) == keys(hi) == 5 and (v[lo], v[hi]) == (cm.KEEP, cm.TIP)
    # fork 4: both short arms go beside the long one
    assert keys(ids[3][2]) == 3 * k + 1 and [v[i] for i in ids[3]] == [cm.TIP, cm.TIP, cm.KEEP]
    # fork 5: the k-key arm goes beside the k+1-key arm, which is no candidate
    assert (keys(ids[4][0]), keys(ids[4][1])) == (k, k + 1) and (v[ids[4][0]], v[ids[4][1]]) == (cm.TIP, cm.KEEP)
    assert ids[4][1] not in c.candidates and ids[3][2] not in c.candidates and len(c.candidates) == 9
    # the model cannot pass vacuously: every level of the comparison decided something, and a candidate survives
    assert all(c.levels[l] > 0 for l in ("not_candidate", "abundance", "keys", "id")), c.levels
    assert any(v[i] == cm.KEEP for i in c.candidates)
    assert c.summary[3] + c.summary[4] + c.summary[5] == u.summary[2] == len(table)
    assert c.summary[4] == 5 * 5 + k and c.summary[7] == sum(c.kept.values())
    assert set(c.kept) == set(table) - {gm.canon(s[j:j + k], canonical) for i, s in enumerate(u.seqs) if v[i] == cm.TIP for j in range(len(s) - k + 1)}


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", KS)
def test_model_on_islands(k, canonical):
    reads, _ = ci.five_forks(k, 100 + k)
    isl = ci.islands(k, 200 + k)
    table = gm.count_table(reads + isl, k, canonical)
    c = cm.clean(table, canonical)
    small, large = (ci.unitig_of(c.unitigs, s, k, canonical) for s in isl)
    assert c.summary[:3] == [18, 6, 1] and c.summary[5] == 3 and c.summary[6] == 9
    assert c.verdict[small] == cm.ISLAND and c.verdict[large] == cm.KEEP and small not in c.candidates
    # the limits: 0 switches a rule off, 2^31 means unlimited
    assert cm.clean(table, canonical, max_tip=k, max_island=0).summary[1:3] == [6, 0]
    assert cm.clean(table, canonical, max_tip=0, max_island=k).summary[1:3] == [0, 1]
    assert cm.clean(table, canonical, max_tip=0, max_island=1 << 31).summary[1:3] == [0, 2]
    assert cm.clean(table, canonical, max_tip=0, max_island=k + 1).summary[1:3] == [0, 2]
    none = cm.clean(table, canonical, max_tip=0, max_island=0)
    assert none.kept == table and none.summary[1:3] == [0, 0] and none.summary[6] == 0
    # unlimited tips: in fork 4 the long arm competes too and wins on its length; in fork 5 the k+1-key arm now wins as a candidate
    assert cm.clean(table, canonical, max_tip=1 << 31, max_island=0).summary[1] == 6


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", KS)
def test_model_compares_wide_products(k, canonical):
    table, arm5, arm6 = ci.wide_fork(k, canonical, 300 + k)
    c = cm.clean(table, canonical)
    u5, u6 = ci.unitig_of(c.unitigs, arm5, k, canonical), ci.unitig_of(c.unitigs, arm6, k, canonical)
    a5, a6 = c.unitigs.abund[u5], c.unitigs.abund[u6]
    assert (a5, a6) == (((1 << 64) - 1) // 6, -(-(1 << 64) // 5) + 7)
    assert (c.verdict[u5], c.verdict[u6]) == (cm.TIP, cm.KEEP) and c.levels["abundance"] == 2
    # what a 64-bit product would have decided
    assert (a6 * 5) % (1 << 64) < (a5 * 6) % (1 << 64)
    assert c.summary[7] == sum(c.kept.values()) < 1 << 64


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", KS)
def test_model_rounds(k, canonical):
    table = gm.count_table(ci.rounds_input(k, 400 + k), k, canonical)
    first = cm.clean(table, canonical)
    assert first.summary[:3] == [7, 2, 1] and first.summary[4:6] == [4 + 5, 3], first.summary
    after = um.unitigs(first.kept, canonical)
    assert sorted(len(s) - k + 1 for s in after.seqs) == sorted([5 * k + 1, k + 6])
    final, words = cm.rounds(table, canonical, n_rounds=4)
    assert len(words) == 2 and words[0] == first.summary and words[1][:3] == [2, 0, 0] and final == first.kept
    assert cm.rounds(table, canonical, n_rounds=1) == (first.kept, [first.summary])
    # a range: the keys outside it are gone after the first round
    final2, words2 = cm.rounds(table, canonical, 2, 0, n_rounds=4)
    assert all(cnt >= 2 for cnt in final2.values()) and len(words2) >= 1


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 7, 8, 21])
def test_model_properties_on_random_reads(k):
    rng = np.random.default_rng(5000 + k)
    for canonical in (True, False):
        for trial in range(2):
            table = gm.count_table(_random_reads(rng, k), k, canonical)
            for lo, hi in ((1, 0), (2, 0), (1, 1)):
                t = um.unitigs(table, canonical, lo, hi).summary
                for tip, isl in ((k, k), (3 * k, 3 * k), (0, 0), (1, 1), (1 << 31, 1 << 31)):
                    c = cm.clean(table, canonical, lo, hi, tip, isl)
                    w = c.summary
                    ctx = (k, canonical, trial, lo, hi, tip, isl)
                    assert w[0] == t[0] and w[3] + w[4] + w[5] == t[2], ctx
                    assert w[1] <= w[6] and w[3] == len(c.kept) and w[7] == sum(c.kept.values()), ctx
                    assert all(c.verdict[u] == cm.KEEP for u, f in enumerate(c.unitigs.flags) if f), ctx
                    if (tip, isl) == (0, 0):
                        solid = gm.solid_set(table, lo, hi)
                        assert c.kept == {x: table[x] for x in solid} and w[1] == w[2] == w[6] == 0, ctx
                    if not canonical or k % 2:
                        # the records from the spelled strings alone give the same verdicts
                        u = c.unitigs
                        offs, to = lm.brute_force(u.seqs, k, canonical)
                        m = [len(s) - k + 1 for s in u.seqs]
                        assert cm.verdicts_from(m, u.abund, u.flags, offs, to, tip, isl)[0] == c.verdict, ctx


def _tool():
    import importlib.util
    spec = importlib.util.spec_from_file_location("measure_clean", os.path.join(ROOT, "tools", "measure_clean.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def model_objects(kmc, table, canonical, c):
    """the package's Table / Unitigs / UnitigLinks objects filled from the model, as tools/measure_clean.host_clean takes them"""
    keys = sorted(table)
    enc = [kmc.encode_key(x, False) for x in keys]
    k = len(keys[0])
    t = kmc.Table(np.array([e[0] for e in enc], np.uint64), np.array([e[1] for e in enc], np.uint64), np.array([table[x] for x in keys], np.uint64), k)
    u, lk = c.unitigs, c.links
    uo = kmc.Unitigs(np.frombuffer(u.bases.encode(), np.uint8), np.array(u.offsets, np.uint64), np.array(u.abund, np.uint64),
                     np.array(u.flags, np.uint8), kmc.UnitigSummary.from_words(u.summary))
    lo = kmc.UnitigLinks(np.array(lk.offsets, np.uint64), np.array(lk.to, np.uint32), kmc.LinkSummary.from_words(lk.summary))
    return t, uo, lo


@pytest.mark.parametrize("canonical", [True, False])
def test_the_measuring_tools_host_computation_agrees_with_the_model(kmc, canonical):
    """tools/measure_clean.py compares the device against numpy on tables no Python model can walk: its numpy is checked here"""
    tool = _tool()
    k = 21
    tables = [gm.count_table(ci.five_forks(k, 100 + k)[0] + ci.islands(k, 200 + k) + ci.rounds_input(k, 400 + k), k, canonical),
              ci.wide_fork(k, canonical, 300 + k)[0],
              gm.count_table(_random_reads(np.random.default_rng(77), k), k, canonical)]
    for table in tables:
        for tip, isl in ((k, k), (0, 0), (1 << 31, 1 << 31), (3 * k, 2)):
            c = cm.clean(table, canonical, 1, 0, tip, isl)
            lo, cnt, verdict, words = tool.host_clean(*model_objects(kmc, table, canonical, c), k, canonical, tip, isl)
            keys = sorted(c.kept)
            assert list(verdict) == c.verdict and words == c.summary
            assert [int(x) for x in lo] == [kmc.encode_key(x, False)[1] for x in keys] and [int(x) for x in cnt] == [c.kept[x] for x in keys]
