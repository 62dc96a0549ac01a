"""Cleaning the compacted graph -- tips clipped, islands dropped -- restated with Python integers on top of
unitig_model.unitigs and links_model.links: the model the clean tests compare kmc_unitig_clean against.  verdicts_from is
the definition of include/kmc.h on plain lists (keys per unitig, abundances, circular flags, link offsets and targets), so
it can also be fed with links found another way (links_model.brute_force)."""
import graph_model as gm
import links_model as lm
import unitig_model as um

FIELDS = ("unitigs", "tips", "islands", "kept_keys", "tip_keys", "island_keys", "tip_candidates", "kept_count")
KEEP, TIP, ISLAND = 0, 1, 2
UNLIMITED = 1 << 31


def _within(m, limit):
    return limit >= UNLIMITED or m <= limit


def verdicts_from(m, abund, flags, offsets, to, max_tip, max_island):
    """(verdict per unitig, the candidates, {comparison level: times it decided}) from m[u] keys, abund[u], flags[u] and the
    records to[offsets[e]:offsets[e + 1]] of end e"""
    nu = len(m)

    def rec(e):
        return to[offsets[e]:offsets[e + 1]]

    def attached(u):
        """the attached end of a tip candidate, None for any other unitig"""
        if flags[u] & 1 or not _within(m[u], max_tip):
            return None
        n0, n1 = len(rec(2 * u)), len(rec(2 * u + 1))
        if (n0, n1) == (0, 1):
            return 2 * u + 1
        if (n0, n1) == (1, 0):
            return 2 * u
        return None

    levels = {"not_candidate": 0, "abundance": 0, "keys": 0, "id": 0}

    def dominates(w, u):
        if attached(w) is None:
            levels["not_candidate"] += 1
            return True
        left, right = abund[w] * m[u], abund[u] * m[w]      # Python integers: exact
        if left != right:
            levels["abundance"] += 1
            return left > right
        if m[w] != m[u]:
            levels["keys"] += 1
            return m[w] > m[u]
        levels["id"] += 1
        return w < u

    verdict, cands = [], []
    for u in range(nu):
        if not flags[u] & 1 and not rec(2 * u) and not rec(2 * u + 1) and _within(m[u], max_island):
            verdict.append(ISLAND)
            continue
        a = attached(u)
        if a is None:
            verdict.append(KEEP)
            continue
        cands.append(u)
        t = rec(a)[0]
        sib = [s >> 1 for s in rec(t) if s != a and s >> 1 != u]
        verdict.append(TIP if any([dominates(w, u) for w in sib]) else KEEP)
    return verdict, cands, levels


class Clean:
    def __init__(self, verdict, cands, levels, kept, summary, unitigs, links):
        self.verdict, self.candidates, self.levels, self.kept, self.summary = verdict, cands, levels, kept, summary
        self.unitigs, self.links = unitigs, links

    @property
    def removed(self):
        return self.summary[1] + self.summary[2]


def clean(table, canonical, min_count=1, max_count=0, max_tip=None, max_island=None, graph=None):
    """The verdicts, the kept {k-mer: count} and the summary words of a table {k-mer string: count}; a limit of None is k.
    graph: (unitig_model.unitigs, links_model.links) of this table and range, if the caller has them already."""
    u, lk = graph or (um.unitigs(table, canonical, min_count, max_count), lm.links(table, canonical, min_count, max_count))
    k = len(next(iter(table))) if table else 0
    max_tip = k if max_tip is None else max_tip
    max_island = k if max_island is None else max_island
    m = [len(s) - k + 1 for s in u.seqs]
    verdict, cands, levels = verdicts_from(m, u.abund, u.flags, lk.offsets, lk.to, max_tip, max_island)
    kept = {}
    for s, v in zip(u.seqs, verdict):
        if v == KEEP:
            for j in range(len(s) - k + 1):
                x = gm.canon(s[j:j + k], canonical)
                kept[x] = table[x]
    keys = [sum(mu for mu, v in zip(m, verdict) if v == c) for c in (KEEP, TIP, ISLAND)]
    assert keys[0] == len(kept) and sum(keys) == u.summary[2]
    summary = [len(m), verdict.count(TIP), verdict.count(ISLAND), keys[0], keys[1], keys[2], len(cands), sum(kept.values())]
    return Clean(verdict, cands, levels, kept, summary, u, lk)


def rounds(table, canonical, min_count=1, max_count=0, max_tip=None, max_island=None, n_rounds=1):
    """(the table after the rounds, [the summary of every round run]): a round cleans the table of the round before with
    the same range; the loop stops after a round that removes nothing."""
    out = []
    for _ in range(n_rounds):
        c = clean(table, canonical, min_count, max_count, max_tip, max_island)
        out.append(c.summary)
        table = c.kept
        if c.removed == 0:
            break
    return table, out


def table_text(table):
    """What the CLI prints for a table: ``KMER\\tCOUNT`` lines in key order."""
    return "".join("%s\t%d\n" % (x, table[x]) for x in sorted(table))
