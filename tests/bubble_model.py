"""Cleaning with simple bubbles popped, restated twice: the model the simplify tests compare kmc_unitig_simplify against.
verdicts_from is the bubble rule of include/kmc.h in Python integers on plain lists, layered on clean_model.verdicts_from
(tips and islands are decided there and are not touched here: the three classes exclude one another by their record
counts).  np_verdicts / np_simplify say the same with numpy arrays, without a line in common with the first: the route
tools/measure_simplify.py takes on tables no Python model can walk."""
import importlib.util
import os

import numpy as np

import clean_model as cm
import graph_model as gm
import links_model as lm
import unitig_model as um

FIELDS = cm.FIELDS + ("bubbles", "bubble_keys", "bubble_candidates", "bubble_count")
KEEP, TIP, ISLAND, BUBBLE = 0, 1, 2, 3
UNLIMITED = cm.UNLIMITED


def verdicts_from(m, abund, flags, offsets, to, max_tip, max_island, max_bubble):
    """(verdict per unitig 0..3, tip candidates, tip levels, bubble candidates, {comparison level: times it decided between
    two parallel arms})"""
    verdict, cands, levels = cm.verdicts_from(m, abund, flags, offsets, to, max_tip, max_island)
    verdict = list(verdict)

    def rec(e):
        return to[offsets[e]:offsets[e + 1]]

    def ends(u):
        """(p, q) of a bubble candidate, None for any other unitig"""
        if flags[u] & 1 or max_bubble == 0 or not cm._within(m[u], max_bubble):
            return None
        r0, r1 = rec(2 * u), rec(2 * u + 1)
        if len(r0) != 1 or len(r1) != 1:
            return None
        p, q = r0[0], r1[0]
        if p == q or p >> 1 == u or q >> 1 == u:
            return None
        return p, q

    blevels = {"abundance": 0, "keys": 0, "id": 0}

    def beats(w, u):
        left, right = abund[w] * m[u], abund[u] * m[w]      # Python integers: exact
        if left != right:
            blevels["abundance"] += 1
            return left > right
        if m[w] != m[u]:
            blevels["keys"] += 1
            return m[w] > m[u]
        blevels["id"] += 1
        return w < u

    bcands = []
    for u in range(len(m)):
        e = ends(u)
        if e is None:
            continue
        assert verdict[u] == KEEP                            # one record at each end: neither a tip nor an island
        bcands.append(u)
        sib = [s >> 1 for s in rec(e[0]) if s >> 1 != u]
        par = [w for w in sib if ends(w) is not None and set(ends(w)) == set(e)]
        if any([beats(w, u) for w in par]):
            verdict[u] = BUBBLE
    return verdict, cands, levels, bcands, blevels


class Simplified:
    def __init__(self, verdict, cands, levels, bcands, blevels, kept, summary, unitigs, links):
        self.verdict, self.candidates, self.levels, self.kept, self.summary = verdict, cands, levels, kept, summary
        self.bubble_candidates, self.bubble_levels = bcands, blevels
        self.unitigs, self.links = unitigs, links

    @property
    def removed(self):
        return self.summary[1] + self.summary[2] + self.summary[8]


def simplify(table, canonical, min_count=1, max_count=0, max_tip=None, max_island=None, max_bubble=None, graph=None):
    """clean_model.clean with the bubble rule: the verdicts, the kept {k-mer: count} and the twelve summary words; a limit
    of None is k.  The counts of a popped arm are not moved onto the survivor."""
    u, lk = graph or (um.unitigs(table, canonical, min_count, max_count), lm.links(table, canonical, min_count, max_count))
    k = len(next(iter(table))) if table else 0
    max_tip = k if max_tip is None else max_tip
    max_island = k if max_island is None else max_island
    max_bubble = k if max_bubble is None else max_bubble
    m = [len(s) - k + 1 for s in u.seqs]
    verdict, cands, levels, bcands, blevels = verdicts_from(m, u.abund, u.flags, lk.offsets, lk.to, max_tip, max_island, max_bubble)
    kept, popped_count = {}, 0
    for s, v in zip(u.seqs, verdict):
        for j in range(len(s) - k + 1):
            x = gm.canon(s[j:j + k], canonical)
            if v == KEEP:
                kept[x] = table[x]
            elif v == BUBBLE:
                popped_count += table[x]
    keys = [sum(mu for mu, v in zip(m, verdict) if v == c) for c in (KEEP, TIP, ISLAND, BUBBLE)]
    assert keys[0] == len(kept) and sum(keys) == u.summary[2]
    summary = [len(m), verdict.count(TIP), verdict.count(ISLAND), keys[0], keys[1], keys[2], len(cands), sum(kept.values()),
               verdict.count(BUBBLE), keys[3], len(bcands), popped_count]
    return Simplified(verdict, cands, levels, bcands, blevels, kept, summary, u, lk)


def rounds(table, canonical, min_count=1, max_count=0, max_tip=None, max_island=None, max_bubble=None, n_rounds=1):
    """(the table after the rounds, [the twelve words of every round run]); the loop stops after a round that removes nothing"""
    out = []
    for _ in range(n_rounds):
        c = simplify(table, canonical, min_count, max_count, max_tip, max_island, max_bubble)
        out.append(c.summary)
        table = c.kept
        if c.removed == 0:
            break
    return table, out


# ---- the same with numpy, on the arrays of kmc_unitigs and kmc_unitig_links ----
U64 = np.uint64


def _measure_clean():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "measure_clean.py")
    spec = importlib.util.spec_from_file_location("measure_clean", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_mc = _measure_clean()


def np_bubbles(offsets, abund, flags, link_offsets, link_to, k, max_bubble):
    """(popped, candidate): two bool arrays per unitig, the bubble rule vectorised"""
    nu = len(abund)
    if not nu or max_bubble == 0:
        return np.zeros(nu, bool), np.zeros(nu, bool)
    m = (np.diff(offsets) - U64(k - 1)).astype(U64)
    lo = link_offsets.astype(np.int64)
    to = np.concatenate([link_to.astype(np.int64), [0]])            # (a pad: index 0..n_links is always readable)
    ids = np.arange(nu)
    one = (np.diff(lo)[0::2] == 1) & (np.diff(lo)[1::2] == 1)
    fits = np.ones(nu, bool) if max_bubble >= UNLIMITED else m <= U64(max_bubble)
    p, q = to[lo[0:2 * nu:2]], to[lo[1:2 * nu:2]]
    cand = one & fits & ((flags & 1) == 0) & (p != q) & ((p >> 1) != ids) & ((q >> 1) != ids)
    popped = np.zeros(nu, bool)
    u = np.flatnonzero(cand)
    pu, qu = p[u], q[u]
    for j in range(4):
        idx = lo[pu] + j
        ok = idx < lo[pu + 1]
        w = to[np.where(ok, idx, 0)] >> 1
        ok &= (w != u) & cand[w] & (((p[w] == pu) & (q[w] == qu)) | ((p[w] == qu) & (q[w] == pu)))
        lh, ll = _mc._mul128(abund[w], m[u])
        rh, rl = _mc._mul128(abund[u], m[w])
        more = (lh > rh) | ((lh == rh) & (ll > rl))
        same = (lh == rh) & (ll == rl)
        popped[u] |= ok & (more | (same & ((m[w] > m[u]) | ((m[w] == m[u]) & (w < u)))))
    return popped, cand


def np_verdicts(offsets, abund, flags, link_offsets, link_to, k, max_tip, max_island, max_bubble):
    verdict = _mc.host_verdicts(offsets, abund, flags, link_offsets, link_to, k, max_tip, max_island)
    popped, cand = np_bubbles(offsets, abund, flags, link_offsets, link_to, k, max_bubble)
    assert not (popped & (verdict != 0)).any()
    verdict[popped] = BUBBLE
    return verdict, cand


def np_simplify(table, unitigs, links, k, canonical, max_tip, max_island, max_bubble):
    """(key_lo, count, verdict, twelve summary words) from Table / Unitigs / UnitigLinks objects of the package, k <= 31"""
    assert k <= 31
    verdict, bcand = np_verdicts(unitigs.offsets, unitigs.abund, unitigs.flags, links.offsets, links.to, k, max_tip, max_island, max_bubble)
    nu = len(verdict)
    if not nu:
        return np.zeros(0, U64), np.zeros(0, U64), verdict, [0] * 12
    code = np.zeros(256, U64)
    code[[ord(c) for c in "ACGT"]] = np.arange(4, dtype=U64)
    c = code[unitigs.bases]
    nb = len(c)
    fwd, rev = np.zeros(nb - k + 1, U64), np.zeros(nb - k + 1, U64)
    for j in range(k):
        x = c[j:nb - k + 1 + j]
        fwd |= x << U64(2 * (k - 1 - j))
        rev |= (U64(3) - x) << U64(2 * j)
    key = np.minimum(fwd, rev) if canonical else fwd
    offs = unitigs.offsets.astype(np.int64)
    m = np.diff(offs) - (k - 1)
    start = np.repeat(offs[:-1], m) + (np.arange(int(m.sum())) - np.repeat(np.cumsum(m) - m, m))
    v_of_key = np.repeat(verdict, m)

    def rows(v):
        ks = np.sort(key[start[v_of_key == v]])
        r = np.searchsorted(table.key_lo, ks)
        assert np.array_equal(table.key_lo[r], ks)
        return ks, table.count[r]

    kept, cnt = rows(KEEP)
    r = np.diff(links.offsets.astype(np.int64))
    fits = m <= max_tip if max_tip < UNLIMITED else np.ones(nu, bool)
    tcand = ((unitigs.flags & 1) == 0) & fits & (((r[0::2] == 0) & (r[1::2] == 1)) | ((r[0::2] == 1) & (r[1::2] == 0)))
    words = [nu, int((verdict == TIP).sum()), int((verdict == ISLAND).sum()), len(kept), int(m[verdict == TIP].sum()),
             int(m[verdict == ISLAND].sum()), int(tcand.sum()), int(cnt.sum(dtype=U64)), int((verdict == BUBBLE).sum()),
             int(m[verdict == BUBBLE].sum()), int(bcand.sum()), int(rows(BUBBLE)[1].sum(dtype=U64))]
    return kept, cnt, verdict, words
