"""The correction rule of include/kmc.h (kmc_correct) as tests/correct_model.py states it, checked against itself: the
independence of the candidates, idempotence, the summary identities, a restatement that corrects one candidate after the
other, and how many injected substitutions the rule recovers.  CPU only."""
import pytest

import correct_inputs as ci
import correct_model as cm
import graph_model as gm


def _cases():
    for k in (5, 31, 32):
        for canonical in (True, False):
            yield k, canonical


@pytest.mark.parametrize("k,canonical", list(_cases()))
def test_candidates_are_independent_and_the_identities_hold(k, canonical):
    sample, reads = ci.genome_reads(k, 7 + k)
    table = gm.count_table(sample, k, canonical)
    for lo, hi in ((1, 0), (2, 0), (2, 3)):
        m = cm.correct_reads(table, canonical, reads, lo, hi)       # (correct_read asserts the window / position claims)
        w = m.summary
        assert w[0] == len(reads) and w[4] == m.cand_offsets[-1] == len(m.cands) and w[5] + w[6] <= w[4] <= w[3]
        assert w[1] == sum(s[0] for s in m.stats) and w[2] == sum(s[1] for s in m.stats) and w[5] == sum(s[3] for s in m.stats)
        assert w[5] == len(m.fixes())
        solid = gm.solid_set(table, lo, hi)
        for r, (a, b) in enumerate(zip(reads, m.corrected)):
            assert len(a) == len(b)
            diff = [i for i in range(len(a)) if a[i] != b[i]]
            recs = m.cands[m.cand_offsets[r]:m.cand_offsets[r + 1]]
            assert diff == [p for p, word, _, _ in recs if (word & 255) != (word >> 8 & 255)]
            # a correction turns exactly its n windows strong and changes no other window
            wa, wb = cm.windows(a, k, canonical, solid), cm.windows(b, k, canonical, solid)
            turned = [j for j in range(len(wa)) if wa[j] != wb[j]]
            want = sorted(j for p, word, s, n in recs if (word & 255) != (word >> 8 & 255) for j in range(s, s + n))
            assert turned == want and all(wb[j] is False for j in turned)
        # correcting the corrected batch again corrects nothing, and its weak windows are the first call's word [7]
        again = cm.correct_reads(table, canonical, m.corrected, lo, hi)
        assert again.corrected == m.corrected and again.summary[5] == 0 and again.summary[2] == w[7]
        # one candidate after the other on the partly corrected read, in either order
        assert cm.sequentially(table, canonical, reads, lo, hi) == m.corrected
        assert cm.sequentially(table, canonical, reads, lo, hi, reverse=True) == m.corrected
    if k >= 31:
        assert cm.correct_reads(table, canonical, reads, 2, 0).summary[5] >= 20


def test_the_placed_errors_by_name():
    k = 31
    for canonical in (True, False):
        sample, reads, names = ci.placed(k, 3)
        m = cm.correct_reads(gm.count_table(sample, k, canonical), canonical, reads, 2, 0)
        L = len(reads[0])
        rec = lambda name: m.cands[m.cand_offsets[names[name]]:m.cand_offsets[names[name] + 1]]
        kinds = lambda name: [(p, w >> 16 & 255, a, n) for p, w, a, n in rec(name)]
        assert kinds("clean") == []
        assert kinds("at_0") == [(0, cm.HEAD, 0, 1)]
        assert kinds("at_k-1") == [(k - 1, cm.HEAD, 0, k)]
        assert kinds("at_k") == [(k, cm.INTERIOR, 1, k)]
        assert kinds("at_L-k-1") == [(L - k - 1, cm.INTERIOR, L - 2 * k, k)]
        assert kinds("at_L-k") == [(L - k, cm.TAIL, L - 2 * k + 1, k)]
        assert kinds("at_L-1") == [(L - 1, cm.TAIL, L - k, 1)]
        assert kinds("two_k+1_apart") == [(k, cm.INTERIOR, 1, k), (2 * k + 1, cm.INTERIOR, k + 2, k)]
        assert kinds("two_k_apart") == [] and kinds("two_k-1_apart") == [] and kinds("weak_end_to_end") == []
        assert kinds("before_N") == []                      # its run ends at the N: INVALID border
        for name in ("at_0", "at_k-1", "at_k", "at_L-k-1", "at_L-k", "at_L-1", "two_k+1_apart"):
            assert m.corrected[names[name]] == reads[0], name
        for name in ("two_k_apart", "two_k-1_apart", "before_N", "weak_end_to_end"):
            assert m.corrected[names[name]] == reads[names[name]], name


def test_ambiguity_and_the_range():
    k = 31
    sample, reads, p, ref, alt = ci.snp(k, 11)
    table = gm.count_table(sample, k, True)
    m = cm.correct_reads(table, True, reads, 2, 0)
    (q, word, a, n), = m.cands[:m.cand_offsets[1]]
    assert q == p and word >> 24 == (1 << "ACGT".index(ref) | 1 << "ACGT".index(alt)) and (word & 255) == (word >> 8 & 255)
    assert m.corrected == reads and m.summary[5:7] == [0, 1]
    m = cm.correct_reads(table, True, reads, 3, 0)
    assert m.corrected[0] == reads[1] and m.summary[5] == 2 and m.corrected[2] == reads[1]    # the variant read goes too


RECOVERY = [(k, 900, 100) for k in (15, 21, 31, 32, 33)] + [(63, 450, 250)]


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k,n_reads,read_len", RECOVERY)
def test_injected_substitutions_are_recovered(k, n_reads, read_len, canonical):
    """The reads themselves are counted, range (2, 0): no clean read is touched, no read becomes anything but its original,
    at least 90 % of the errors are restored"""
    reads, orig, where = ci.recovery(k, 100 + k, n_reads, read_len)
    m = cm.correct_reads(gm.count_table(reads, k, canonical), canonical, reads, 2, 0)
    n_err = sum(w is not None for w in where)
    restored = 0
    for r, s, o, w in zip(reads, m.corrected, orig, where):
        if w is None:
            assert s == r
        else:
            assert s in (r, o)
            restored += s == o
    print("k %d canonical %d: %d of %d restored (%.1f %%), ambiguous %d" % (k, canonical, restored, n_err, 100.0 * restored / n_err, m.summary[6]))
    assert restored >= 0.9 * n_err
