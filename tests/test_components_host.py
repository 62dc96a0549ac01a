"""CPU-side checks of the connected components of the unitig graph: the model the GPU tests compare against
(tests/components_model.py) against its independent brute force over the keys and against its numpy restatement on every
hand-built input of components_inputs.py, the identities of include/kmc.h on the model, the inclusion of the island rule,
the header section, the exported symbols and their argument rules without a device, the Python binding, and the CLI's
argument errors, which end before a GPU is touched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import clean_model as cm
import components_inputs as xi
import components_model as xm
import graph_model as gm
import links_model as lm
import unitig_model as um
from conftest import ROOT, SAMPLE

NEW = ("kmc_unitig_components", "kmc_unitig_components_device", "kmc_unitig_components_into")
EXE = os.path.join(ROOT, "bin", "k-mer-count")
BIG = 1 << 31
_CACHE = {}


def _models(k, canonical):
    """{name: (table, unitigs, links)} of the built inputs, computed once per (k, canonical)"""
    if (k, canonical) not in _CACHE:
        out = {}
        for name, reads in xi.built(k).items():
            table = gm.count_table(reads, k, canonical)
            out[name] = (table, um.unitigs(table, canonical), lm.links(table, canonical))
        _CACHE[(k, canonical)] = out
    return _CACHE[(k, canonical)]


# no key is its own reverse complement: a forward ctx, or canonical with odd k
SYMMETRIC = ((5, False), (12, False), (31, False), (5, True), (13, True), (31, True))


@pytest.mark.parametrize("k,canonical", SYMMETRIC)
def test_model_against_the_brute_force_over_the_keys(k, canonical):
    for name, (table, u, lk) in _models(k, canonical).items():
        c = xm.components(table, canonical, graph=(u, lk))
        assert c.comp_of == xm.brute_force(table, canonical), (name, k, canonical)
        assert [s[0] for s in c.stats] == sorted(s[0] for s in c.stats) and (not c.stats or c.stats[0][0] == 0)
        assert all(s[0] == min(c.members(i)) for i, s in enumerate(c.stats))
    # a count range: the unitigs and links of the solid keys alone
    table = _models(k, canonical)["rounds_input"][0]
    assert xm.components(table, canonical, 2, 0).comp_of == xm.brute_force(table, canonical, 2, 0)


@pytest.mark.parametrize("k,canonical", SYMMETRIC + ((32, True), (6, True)))
def test_identities_and_the_numpy_form(k, canonical):
    for name, (table, u, lk) in _models(k, canonical).items():
        m = [len(s) - k + 1 for s in u.seqs]
        for limit in (0, 1, k, k + 3, k + 4, BIG):
            c = xm.components(table, canonical, limit=limit, graph=(u, lk))
            ctx = (name, k, canonical, limit)
            assert sum(s[1] for s in c.stats) == c.summary[0] == u.summary[0], ctx
            assert sum(s[2] for s in c.stats) == u.summary[2] and sum(s[3] for s in c.stats) == u.summary[7], ctx
            assert c.summary[2] >= lk.summary[6], ctx
            assert c.summary[1] == len(c.stats) == (max(c.comp_of) + 1 if c.comp_of else 0), ctx
            if limit == 0:
                assert c.kept == {x: n for x, n in table.items()} and c.summary[5] == 0, ctx
            if limit == BIG:
                assert c.kept == {} and c.summary[5] == c.summary[1], ctx
            assert set(c.verdict) <= {xm.KEEP, xm.COMPONENT}
            got = xm.np_components(np.array(lk.offsets, np.uint64), np.array(lk.to, np.uint32), np.array(m, np.uint64),
                                   np.array(u.abund, np.uint64), limit)
            assert got[0].tolist() == c.comp_of and got[1].tolist() == c.stats and got[2].tolist() == c.verdict, ctx
            # every island of the clean rule is a small component under the same limit
            isl = cm.clean(table, canonical, 1, 0, 0, limit, graph=(u, lk))
            assert all(c.verdict[i] == xm.COMPONENT for i, v in enumerate(isl.verdict) if v == cm.ISLAND), ctx


def test_the_built_inputs_are_what_they_say():
    k = 31
    for canonical in (True, False):
        mod = _models(k, canonical)
        res = {name: xm.components(t, canonical, graph=(u, lk)) for name, (t, u, lk) in mod.items()}
        assert res["ladder"].summary[:3] == [121, 1, 0]
        assert res["islands_and_fork"].summary[0] == 303 and res["islands_and_fork"].summary[1:3] == [301, 300]
        assert res["comb"].summary[:2] == [141, 1]
        # components of exactly k + 3 and k + 4 keys, and the fork of k + 11
        assert sorted(s[2] for s in res["boundary"].stats) == [k + 3, k + 4, k + 11]
        for limit, small in ((k + 2, 0), (k + 3, 1), (k + 4, 2), (k + 10, 2), (k + 11, 3)):
            t, u, lk = mod["boundary"]
            assert xm.components(t, canonical, limit=limit, graph=(u, lk)).summary[5] == small
        # the circular read: one unitig, one self record, a component that IS small (an island it is not)
        t, u, lk = mod["circular"]
        cu = [i for i, f in enumerate(u.flags) if f]
        assert len(cu) == 1 and lk.summary[4] >= 1
        c = xm.components(t, canonical, limit=2 * k, graph=(u, lk))
        assert c.verdict[cu[0]] == xm.COMPONENT and c.stats[c.comp_of[cu[0]]][1:3] == [1, 2 * k]
        assert cm.clean(t, canonical, 1, 0, 0, 2 * k, graph=(u, lk)).verdict[cu[0]] == cm.KEEP
        # two forks: component 0 holds unitig 0, whichever fork that is, and the sizes differ
        st = res["two_forks"].stats
        assert len(st) == 2 and st[0][0] == 0 and {s[1] for s in st} == {3} and sorted(s[2] for s in st) == [k + 16, 7 * k + 8]
    assert lm.links(*[_models(k, True)["hairpin"][0], True]).summary[4] >= 1          # the hairpin's self record


def test_rounds_remove_nothing_more_the_second_time():
    k = 21
    table = gm.count_table(xi.built(k)["rounds_input"] + xi.built(k)["boundary"], k, True)
    final, words = xm.rounds(table, True, limit=k + 3, n_rounds=4)
    assert len(words) == 2 and words[0][5] >= 2 and words[1][5] == 0 and words[1][0] == words[0][0] - words[0][5]
    assert final == xm.components(table, True, limit=k + 3).kept


def test_header_declares_the_components_section():
    hdr = open(os.path.join(ROOT, "include", "kmc.h")).read()
    for d in ("#define KMC_COMPONENT_WORDS 8", "#define KMC_COMPONENT_STAT_WORDS 4", "#define KMC_CLEAN_COMPONENT 4"):
        assert d in hdr, d
    flat = " ".join(hdr.replace(" * ", " ").split())
    for phrase in ("ADJACENT.", "COMPONENT.", "ROOT.", "NUMBERING.", "SMALL.", "NO exemption for circular unitigs",
                   "A components call counts as a kmc_unitig_links* call", "kmc_unitig_components: keys N unitigs U records R components C"):
        assert phrase in flat, phrase
    for s in NEW:
        assert ("int %s(" % s) in hdr and s in hdr.split("Conventions")[0], s


def test_library_exports_and_binding(kmc):
    out = subprocess.run(["nm", "-D", "--defined-only", kmc.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for s in NEW:
        assert f" T {s}\n" in out, s
        assert s in kmc.ABI_SYMBOLS
    L = kmc.lib()
    vp, u64, pu64 = C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)
    assert L.kmc_unitig_components_device.argtypes == [vp, u64, u64, u64] + [C.POINTER(vp)] * 6 + [pu64, pu64, pu64, vp]
    assert L.kmc_unitig_components.argtypes == [vp, u64, u64, u64, vp, vp, u64, vp, u64, vp, vp, vp, u64, pu64, pu64, pu64, vp]
    assert L.kmc_unitig_components_into.argtypes == [vp, vp, u64, u64, u64, vp]
    a = np.full(16, 7, np.uint64)
    p = a.ctypes.data
    n = [C.c_uint64(7) for _ in range(3)]
    # a NULL ctx: KMC_ERR_ARG, the sizes zeroed, nothing written
    assert L.kmc_unitig_components(None, 1, 0, 5, p, p, 2, p, 2, p, p, p, 2, *[C.byref(x) for x in n], p) == kmc.ERR_ARG
    assert [x.value for x in n] == [0, 0, 0] and (a == 7).all()
    assert L.kmc_unitig_components_device(None, 1, 0, 5, *([None] * 10)) == kmc.ERR_ARG
    assert L.kmc_unitig_components_into(None, None, 1, 0, 5, None) == kmc.ERR_ARG
    assert (kmc.COMPONENT_WORDS, kmc.COMPONENT_STAT_WORDS, kmc.CLEAN_COMPONENT) == (8, 4, 4) == (len(xm.FIELDS), 4, xm.COMPONENT)
    s = kmc.ComponentSummary.from_words(range(8))
    assert s.words() == list(range(8)) and s.small == 5 and s.removed == 5 and s.to_text().splitlines()[1] == "components\t1"
    r = kmc.Components(np.array([0, 1, 0], np.uint32), np.array([[0, 2, 9, 30], [1, 1, 4, 4]], np.uint64), np.zeros(3, np.uint8), None, s)
    assert r.members(0).tolist() == [0, 2] and r.members(1).tolist() == [1] and r.to_text() == "0\t0\t2\t9\t30\n1\t1\t1\t4\t4\n"
    for name in ("components", "components_device", "components_into"):
        assert callable(getattr(kmc.KmerCounter, name))


def test_cli_argument_errors_end_before_the_gpu(kmc):
    run = lambda *a: subprocess.run([EXE, SAMPLE] + list(a), capture_output=True, text=True)
    for args, word in ((("--component-keys", "5"), "needs -k K"), (("--components",), "needs -k K"),
                       (("-k", "21", "--components", "--gfa"), "exclude each other"),
                       (("-k", "21", "--components", "--unitigs"), "exclude each other"),
                       (("-k", "21", "--components", "--graph-stats"), "exclude each other"),
                       (("-k", "21", "--component-keys", "5", "--with", SAMPLE, "--setop", "union"), "exclude each other"),
                       (("-k", "21", "--component-keys", "5", "--with", SAMPLE, "--compare"), "exclude each other"),
                       (("-k", "21", "--component-keys"), "needs a value"), (("-k", "21", "--component-keys", "-1"), "whole number")):
        r = run(*args)
        assert r.returncode == 2 and r.stdout == "" and word in r.stderr, (args, r.returncode, r.stderr)
    r = run("--help")
    assert r.returncode == 0 and "--components" in r.stderr and "--component-keys N" in r.stderr
