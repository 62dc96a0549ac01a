"""Bubbles reported as variant records, restated in plain Python on the unitigs of unitig_model.py and the links of
links_model.py: the model the bubble-call tests compare kmc_unitig_bubbles against.  It follows the bubbles block of
include/kmc.h sentence by sentence -- candidate, parallel, major arm, oriented arms, difference, kind -- on Python strings
and integers, and asserts two things of every input on the way: the oriented arms of a record begin with the same k - 1
bases and end with the same k - 1 bases, and the number of records is what bubble_model.simplify pops with tip and island
limits 0."""
import bubble_model as bm
import graph_model as gm
import links_model as lm
import unitig_model as um

FIELDS = ("unitigs", "records", "candidates", "substitutions", "indels", "complex", "reversed", "called_keys")
SUBST, INDEL, COMPLEX, REVERSED = 0, 1, 2, 4
TOO_LARGE = 1 << 31


class Calls:
    def __init__(self, records, summary, arms, unitigs, links, k):
        self.records, self.summary, self.arms, self.unitigs, self.links, self.k = records, summary, arms, unitigs, links, k

    def alleles(self):
        """(alt, major) per record"""
        return [(U[r[4]:len(U) - r[5]], W[r[4]:len(W) - r[5]]) for r, (U, W) in zip(self.records, self.arms)]

    def text(self):
        """the lines of `k-mer-count --variants`"""
        keys = lambda x: len(self.unitigs.seqs[x]) - self.k + 1
        out = []
        for i, (r, (alt, major)) in enumerate(zip(self.records, self.alleles())):
            out.append("%d\t%s\t%d\t%d\t%d\t%s\t%s\t%d/%d\t%d/%d\n" % (i, {SUBST: "S", INDEL: "I", COMPLEX: "C"}[r[6] & 3], r[0], r[1], r[4], alt or "-",
                                                                     major or "-", self.unitigs.abund[r[0]], keys(r[0]), self.unitigs.abund[r[1]], keys(r[1])))
        return "".join(out)


def _common(a, b, most):
    n = 0
    while n < most and a[n] == b[n]:
        n += 1
    return n


def difference(U, W):
    """(lcp, lcs, mism, kind) of two oriented arms"""
    short = min(len(U), len(W))
    lcp = _common(U, W, short)
    lcs = _common(U[::-1], W[::-1], short - lcp)
    mism = sum(1 for a, b in zip(U, W) if a != b) if len(U) == len(W) else 0
    alt, major = U[lcp:len(U) - lcs], W[lcp:len(W) - lcs]
    if len(U) == len(W) and mism == 1:
        kind = SUBST
    elif (alt == "") != (major == ""):
        kind = INDEL
    else:
        kind = COMPLEX
    return lcp, lcs, mism, kind


def calls(table, canonical, min_count=1, max_count=0, max_bubble=None, graph=None):
    """The records (lists of eight integers, ascending u), the eight summary words and the oriented arms (U, W) of every
    record; a limit of None is k, one of 2^31 or more is a ValueError (KMC_ERR_ARG)."""
    u, lk = graph or (um.unitigs(table, canonical, min_count, max_count), lm.links(table, canonical, min_count, max_count))
    k = len(next(iter(table))) if table else 0
    limit = k if max_bubble is None else max_bubble
    if limit >= TOO_LARGE:
        raise ValueError("max_bubble_keys of 2^31 or more")
    nu = len(u.seqs)
    keys = [len(s) - k + 1 for s in u.seqs]
    records_of = lambda e: lk.to[lk.offsets[e]:lk.offsets[e + 1]]

    def ends(x):
        if u.flags[x] & 1 or keys[x] > limit:
            return None
        start, end = records_of(2 * x), records_of(2 * x + 1)
        if len(start) != 1 or len(end) != 1:
            return None
        p, q = start[0], end[0]
        return None if p == q or p >> 1 == x or q >> 1 == x else (p, q)

    def beats(w, x):
        if u.abund[w] * keys[x] != u.abund[x] * keys[w]:
            return u.abund[w] * keys[x] > u.abund[x] * keys[w]
        return keys[w] > keys[x] if keys[w] != keys[x] else w < x

    records, arms, candidates = [], [], 0
    for x in range(nu):
        e = ends(x)
        if e is None:
            continue
        candidates += 1
        parallel = sorted({s >> 1 for s in records_of(e[0]) if s >> 1 != x and ends(s >> 1) is not None and set(ends(s >> 1)) == set(e)})
        if not parallel:
            continue
        major = [w for w in parallel if all(beats(w, v) for v in parallel if v != w)]
        assert len(major) == 1                                  # the order is strict and total
        w = major[0]
        if not beats(w, x):
            continue
        U, W, flag = u.seqs[x], u.seqs[w], 0
        if records_of(2 * w)[0] != e[0]:
            W, flag = gm.revcomp(W), REVERSED
        assert U[:k - 1] == W[:k - 1] and U[len(U) - (k - 1):] == W[len(W) - (k - 1):], (x, w, U, W)
        lcp, lcs, mism, kind = difference(U, W)
        records.append([x, w, e[0], e[1], lcp, lcs, kind | flag, mism])
        arms.append((U, W))
    kinds = [r[6] & 3 for r in records]
    summary = [nu, len(records), candidates, kinds.count(SUBST), kinds.count(INDEL), kinds.count(COMPLEX),
               sum(1 for r in records if r[6] & REVERSED), sum(keys[r[0]] for r in records)]
    popped = bm.simplify(table, canonical, min_count, max_count, 0, 0, limit, graph=(u, lk))
    assert len(records) == popped.summary[8] and summary[2] == popped.summary[10] and summary[7] == popped.summary[9]
    assert [r[0] for r in records] == [x for x, v in enumerate(popped.verdict) if v == bm.BUBBLE]
    return Calls(records, summary, arms, u, lk, k)
