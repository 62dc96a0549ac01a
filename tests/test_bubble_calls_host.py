"""CPU-side checks of the bubble calls: the two kmc_unitig_bubbles* entry points are exported and keep their argument rules
without a device, the header section and its constants, the CLI knows --variants and rejects bad combinations before touching
a GPU, BubbleSummary / Bubbles, and the model the GPU tests compare against (tests/bubble_call_model.py) on inputs whose
answer is known from how bubble_inputs.py builds them."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bubble_call_model as bcm
import bubble_inputs as bi
import bubble_model as bm
import graph_model as gm
from clean_inputs import rnd
from conftest import ROOT, SAMPLE

NEW = ("kmc_unitig_bubbles", "kmc_unitig_bubbles_device")
EXE = os.path.join(ROOT, "bin", "k-mer-count")
MODES = (True, False)
# bubble_inputs.everything(k, seed) with the seed drawn again until the model gives nine records at limit k + 1 and, in a
# canonical ctx, a reversed arm among them
EVERYTHING_SEED = {31: 121, 32: 123, 63: 153}


def run_deletion(k, seed):
    """(reads, s, the read with the deletion): a sequence of 6k bases with ``C AAA G`` at 3k - 1, read three times, and one
    read of the same stretch with one A of the run missing.  Where the deleted base sits in the run cannot be told: the
    common prefix takes all of ``CAA`` and the cap on the common suffix binds."""
    rng = np.random.default_rng(seed)
    while True:
        left, right = rnd(rng, 3 * k - 1), rnd(rng, 3 * k - 4)
        s, d = left + "CAAAG" + right, left + "CAAG" + right
        if left[-1] != "A" and bi._plain([s, d[len(left) + 4 - (k - 1):len(left) + k - 1]], k):   # (the second piece: the (k-1)-mers that hold CAAG)
            return [s] * 3 + [d[len(left) - k:len(left) + 4 + k]], s, d


def test_library_exports_the_bubble_calls(kmc):
    out = subprocess.run(["nm", "-D", "--defined-only", kmc.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for s in NEW:
        assert f" T {s}\n" in out, s
        assert s in kmc.ABI_SYMBOLS
    L = kmc.lib()
    vp, u64, pu64 = C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)
    assert L.kmc_unitig_bubbles_device.argtypes == [vp, u64, u64, u64, C.POINTER(vp), pu64, pu64, vp]
    assert L.kmc_unitig_bubbles.argtypes == [vp, u64, u64, u64, vp, u64, pu64, pu64, vp]
    a = np.full(8, 7, np.uint64)
    n1, n2 = C.c_uint64(7), C.c_uint64(7)
    # a NULL ctx: KMC_ERR_ARG, the sizes zeroed, nothing written
    assert L.kmc_unitig_bubbles(None, 1, 0, 5, a.ctypes.data, 2, C.byref(n1), C.byref(n2), a.ctypes.data) == kmc.ERR_ARG
    assert n1.value == 0 and n2.value == 0 and (a == 7).all()
    assert L.kmc_unitig_bubbles(None, 1, 0, 5, None, 0, None, None, None) == kmc.ERR_ARG
    assert L.kmc_unitig_bubbles_device(None, 1, 0, 5, None, None, None, None) == kmc.ERR_ARG
    assert kmc.BUBBLE_WORDS == 8 == len(bcm.FIELDS) and kmc.BUBBLE_RECORD_WORDS == 8
    assert (kmc.BUBBLE_SUBST, kmc.BUBBLE_INDEL, kmc.BUBBLE_COMPLEX, kmc.BUBBLE_REVERSED) == (bcm.SUBST, bcm.INDEL, bcm.COMPLEX, bcm.REVERSED)


def test_header_declares_the_bubbles_section():
    hdr = open(os.path.join(ROOT, "include", "kmc.h")).read()
    for line in ("#define KMC_BUBBLE_WORDS 8", "#define KMC_BUBBLE_RECORD_WORDS 8", "#define KMC_BUBBLE_SUBST 0u", "#define KMC_BUBBLE_INDEL 1u",
                 "#define KMC_BUBBLE_COMPLEX 2u", "#define KMC_BUBBLE_REVERSED 4u"):
        assert line in hdr, line
    flat = " ".join(hdr.replace(" * ", " ").split())
    for phrase in ("MAJOR ARM.", "ORIENTED ARMS.", "DIFFERENCE.", "KIND.", "RECORD.", "u is CALLED iff major(u) beats u",
                   "max_bubble_keys of 2^31 or more is KMC_ERR_ARG here", "A bubbles call counts as a kmc_unitig_links* call",
                   "kmc_unitig_bubbles: keys N unitigs U candidates C records R", "pair_ms .. diff_ms .."):
        assert phrase in flat, phrase
    assert "kmc_unitig_bubbles / kmc_unitig_bubbles_device" in hdr.split("Conventions")[0]


@pytest.mark.parametrize("argv", [
    ["--variants"],                                                                        # without -k
    ["-k", "5", "--variants", "--gfa"], ["-k", "5", "--variants", "--components"], ["-k", "5", "--variants", "--histo", "4"],
    ["-k", "5", "--variants", "--expand"], ["-k", "5", "--variants", "--map", SAMPLE], ["-k", "5", "--variants", "--bubble-keys", "x"],
    ["-k", "5", "--variants", "--bubble-keys", str(1 << 31)], ["-k", "5", "--variants", "--tip-keys", "3"],
    ["-k", "5", "--variants", "--with", SAMPLE, "--compare"]])
def test_cli_rejects_bad_variants_options(kmc, argv):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")   # no GPU to touch even where there is one
    r = subprocess.run([EXE, SAMPLE] + argv, capture_output=True, text=True, env=env)
    assert r.returncode == 2 and r.stdout == "" and "k-mer-count:" in r.stderr, (argv, r.returncode, r.stderr)
    assert "unknown option" not in r.stderr, r.stderr


def test_cli_help_lists_variants(kmc):
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "" and "--variants [--bubble-keys N]" in r.stderr


def test_bubble_objects(kmc):
    w = [9, 2, 5, 1, 1, 0, 1, 11]
    s = kmc.BubbleSummary.from_words(np.array(w, np.uint64))
    assert s.words() == w and (s.records, s.candidates, s.substitutions, s.indels, s.complex, s.reversed, s.called_keys) == (2, 5, 1, 1, 0, 1, 11)
    assert s.to_text().splitlines()[:2] == ["unitigs\t9", "records\t2"] and len(s.to_text().splitlines()) == 8
    # three unitigs at k = 3: AACGT (abundance 9, the major arm), AAGGT (called, a substitution), ACCTT (called, W reversed: AAGGT)
    bases = np.frombuffer(b"AACGTAAGGTACCTT", np.uint8)
    u = kmc.Unitigs(bases, np.array([0, 5, 10, 15], np.uint64), np.array([9, 3, 4], np.uint64), np.zeros(3, np.uint8), None)
    rec = np.array([[1, 0, 7, 8, 2, 2, kmc.BUBBLE_SUBST, 1], [2, 1, 7, 8, 1, 1, kmc.BUBBLE_COMPLEX | kmc.BUBBLE_REVERSED, 3]], np.uint32)
    b = kmc.Bubbles(rec, s, u, 3)
    assert len(b) == 2 and b.arms() == [("AAGGT", "AACGT"), ("ACCTT", "ACCTT")]
    assert b.alleles() == [("G", "C"), ("CCT", "CCT")]
    assert b.to_text() == "0\tS\t1\t0\t2\tG\tC\t3/3\t9/3\n1\tC\t2\t1\t1\tCCT\tCCT\t4/3\t3/3\n"
    assert kmc.Bubbles(rec[:0], s, u, 3).to_text() == ""


@pytest.mark.parametrize("canonical", MODES)
@pytest.mark.parametrize("k", [5, 31, 32, 63])
def test_substitution_is_one_subst_record(k, canonical):
    reads, s, err = bi.substitution(k, 10 + k)
    table = gm.count_table(reads, k, canonical)
    c = bcm.calls(table, canonical)
    assert c.summary == [4, 1, 2, 1, 0, 0, c.records[0][6] >> 2, k] and len(c.records) == 1
    u, w, p, q, lcp, lcs, flags, mism = c.records[0]
    assert (flags & 3, lcp, lcs, mism) == (bcm.SUBST, k - 1, k - 1, 1)
    assert u == bi.unitig_with(c.unitigs, err[:k], k, canonical) and w == bi.unitig_with(c.unitigs, s[2 * k + 1:3 * k + 1], k, canonical)
    alt, major = c.alleles()[0]
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    # the alt arm is the error read's, spelled along the read or against it
    assert {alt, major} in ({err[k - 1], s[3 * k]}, {comp[err[k - 1]], comp[s[3 * k]]})
    assert c.unitigs.seqs[u] in (err, gm.revcomp(err)) and (alt == err[k - 1]) == (c.unitigs.seqs[u] == err)
    assert c.text() == "0\tS\t%d\t%d\t%d\t%s\t%s\t%d/%d\t%d/%d\n" % (u, w, k - 1, alt, major, k, k, 3 * k, k)
    # limits: one key too few for the arms, and none at all
    assert bcm.calls(table, canonical, max_bubble=k - 1).summary == [4, 0, 0, 0, 0, 0, 0, 0]
    assert bcm.calls(table, canonical, max_bubble=0).records == []
    with pytest.raises(ValueError):
        bcm.calls(table, canonical, max_bubble=1 << 31)


@pytest.mark.parametrize("canonical", MODES)
@pytest.mark.parametrize("k", [31, 32, 63])
def test_arms_of_k_and_k_plus_1_keys(k, canonical):
    reads, s, e1, e2 = bi.arms_k_and_k_plus_1(k, 30 + k)
    table = gm.count_table(reads, k, canonical)
    assert bcm.calls(table, canonical).summary[1:6] == [1, 2, 1, 0, 0]          # limit k: the arms of k + 1 keys are no candidates
    c = bcm.calls(table, canonical, max_bubble=k + 1)
    assert c.summary[1:6] == [2, 4, 1, 0, 1] and c.summary[7] == 2 * k + 1
    by_kind = {r[6] & 3: r for r in c.records}
    assert by_kind[bcm.SUBST][4:6] == [k - 1, k - 1] and by_kind[bcm.SUBST][7] == 1
    assert by_kind[bcm.COMPLEX][4:6] == [k - 1, k - 1] and by_kind[bcm.COMPLEX][7] == 2
    assert [len(a) for a in c.alleles()[c.records.index(by_kind[bcm.COMPLEX])]] == [2, 2]
    assert by_kind[bcm.COMPLEX][0] == bi.unitig_with(c.unitigs, e2[:k], k, canonical)


@pytest.mark.parametrize("canonical", MODES)
@pytest.mark.parametrize("k", [31, 32, 63])
def test_decided_pairs_hold_an_indel(k, canonical):
    reads, errs = bi.decided_pairs(k, 40 + k)
    c = bcm.calls(gm.count_table(reads, k, canonical), canonical)
    assert c.summary[1:6] == [3, 6, 2, 1, 0]
    r = [x for x in c.records if x[6] & 3 == bcm.INDEL][0]
    alt, major = c.alleles()[c.records.index(r)]
    assert sorted([len(alt), len(major)]) == [0, 1] and r[7] == 0 and r[4] + r[5] == min(len(U) for U in c.arms[c.records.index(r)]) - (0 if "" in (alt, major) else 1)
    # the keys decide that pair: the arm of k keys (the insertion) stays, the true arm of k - 1 keys is the one called
    assert len(c.unitigs.seqs[r[0]]) == 2 * k - 2 and len(c.unitigs.seqs[r[1]]) == 2 * k - 1 and (alt, len(major)) == ("", 1)


@pytest.mark.parametrize("canonical", MODES)
@pytest.mark.parametrize("k", [31, 32, 63])
def test_three_arms_share_their_major(k, canonical):
    reads, s, errs = bi.three_arms(k, 20 + k)
    c = bcm.calls(gm.count_table(reads, k, canonical), canonical)
    assert c.summary[1:6] == [2, 3, 2, 0, 0] and c.records[0][1] == c.records[1][1]
    assert c.records[0][1] == bi.unitig_with(c.unitigs, s[2 * k + 1:3 * k + 1], k, canonical)
    assert {r[0] for r in c.records} == {bi.unitig_with(c.unitigs, e[:k], k, canonical) for e in errs}
    assert c.records[0][0] < c.records[1][0] and all(set(r[2:4]) == set(c.records[0][2:4]) for r in c.records)   # (an arm spelled the other way round has p and q swapped)


@pytest.mark.parametrize("canonical", MODES)
@pytest.mark.parametrize("k", [31, 32, 63])
def test_deletion_in_a_run_binds_the_cap(k, canonical):
    reads, s, d = run_deletion(k, 700 + k)
    c = bcm.calls(gm.count_table(reads, k, canonical), canonical)
    assert c.summary[1:6] == [1, 2, 0, 1, 0]
    u, w, p, q, lcp, lcs, flags, mism = c.records[0]
    U, W = c.arms[0]
    assert (len(U), len(W)) == (2 * k - 4, 2 * k - 3) and lcp + lcs == min(len(U), len(W)) and mism == 0
    assert (lcp, lcs) == (k - 1, k - 3) and c.alleles()[0] in (("", "A"), ("", "T"))
    # uncapped the common suffix would reach into the common prefix: the two A of the run that are left
    rest = 0
    while rest < len(U) and U[len(U) - 1 - rest] == W[len(W) - 1 - rest]:
        rest += 1
    assert rest > lcs
    if k == 31:
        assert (lcp, lcs) == (30, 28)


@pytest.mark.parametrize("canonical", MODES)
@pytest.mark.parametrize("k", [31, 32, 63])
def test_everything_has_nine_records(k, canonical):
    c = bcm.calls(gm.count_table(bi.everything(k, EVERYTHING_SEED[k]), k, canonical), canonical, max_bubble=k + 1)
    assert c.summary[1] == 9 == len(c.records) and [r[0] for r in c.records] == sorted(r[0] for r in c.records)
    assert c.summary[3] + c.summary[4] + c.summary[5] == 9 and c.summary[4] == 1 and c.summary[5] == 1
    if canonical:
        assert 0 < c.summary[6]
    else:
        assert c.summary[6] == 0                                  # a forward ctx spells every arm along the reads


def test_model_agrees_with_simplify_on_the_sample(kmc):
    bases, offs = kmc.parse_fasta(SAMPLE)
    text = bases.tobytes().decode()
    reads = [text[int(a):int(b)] for a, b in zip(offs[:-1], offs[1:])]
    for k, canonical in ((21, True), (32, False)):
        table = gm.count_table(reads, k, canonical)
        for lim in (k, 3 * k):
            c = bcm.calls(table, canonical, max_bubble=lim)
            assert c.summary[1] == bm.simplify(table, canonical, 1, 0, 0, 0, lim).summary[8]
