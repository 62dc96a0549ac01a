"""Read walks counted per graph element, restated in plain Python on top of map_model.py (the segments of every read) and
links_model.py (the records of every unitig end): the model the transit tests compare kmc_unitig_transits against.  It
follows the definitions of include/kmc.h literally -- CROSSING, LINK SUPPORT, TRANSIT, TRANSIT MATRIX, VERDICT -- over Python
lists, read by read, and shares no code with the library."""
import links_model as lm
import map_model as mm
import unitig_model as um

FIELDS = ("crossings", "crossings_without_record", "records_unsupported", "transits", "transits_dropped", "repeats", "resolved", "ambiguous")
PLAIN, UNSPANNED, RESOLVED, AMBIGUOUS = 0, 1, 2, 3
VERDICT_NAMES = ("plain", "unspanned", "resolved", "ambiguous")


class Transits:
    def __init__(self, lk, n_unitigs, k):
        self.lk, self.n_unitigs, self.k = lk, n_unitigs, k
        off = lk.offsets
        assert len(off) == 2 * n_unitigs + 1
        self.d_start = [off[2 * u + 1] - off[2 * u] for u in range(n_unitigs)]
        self.d_end = [off[2 * u + 2] - off[2 * u + 1] for u in range(n_unitigs)]
        self.transit_offsets = [0]
        for u in range(n_unitigs):
            self.transit_offsets.append(self.transit_offsets[-1] + self.d_start[u] * self.d_end[u])
        self.link_support = [0] * len(lk.to)
        self.transit_count = [0] * self.transit_offsets[-1]
        self.totals = [0, 0, 0, 0]          # summary words [0], [1], [3], [4]
        self.loops = 0                      # crossings with a == b
        self.transit_segments = []          # (read, segment record) of every stored transit
        self.verdict, self.summary = [], [0] * 8
        for e in range(2 * n_unitigs):      # "the record e -> t" is well defined
            t = lk.to[off[e]:off[e + 1]]
            assert len(set(t)) == len(t), (e, t)

    def record(self, e, t):
        """index of the record e -> t, or None"""
        off = self.lk.offsets
        for j in range(off[e], off[e + 1]):
            if self.lk.to[j] == t:
                return j
        return None

    def add(self, read_segments):
        """one batch: per read its list of (start, len, uni, pos)"""
        off = self.lk.offsets
        for r, segs in enumerate(read_segments):
            cross = [i > 0 and segs[i][0] == segs[i - 1][0] + segs[i - 1][1] for i in range(len(segs))]
            for i, s in enumerate(segs):
                if not cross[i]:
                    continue
                a, b = segs[i - 1][2] ^ 1, s[2]
                self.totals[0] += 1
                self.loops += a == b
                j1, j2 = self.record(a, b), self.record(b, a) if a != b else None
                if j1 is None and j2 is None:
                    self.totals[1] += 1
                for j in (j1, j2):
                    if j is not None:
                        self.link_support[j] += 1
                if i + 1 < len(segs) and cross[i + 1]:
                    v, o = s[2] >> 1, s[2] & 1
                    e_in, e_out, nxt = 2 * v + o, 2 * v + 1 - o, segs[i + 1][2]
                    jp, jq = self.record(e_in, a), self.record(e_out, nxt)
                    if jp is None or jq is None:
                        self.totals[3] += 1
                        continue
                    p, q = jp - off[e_in], jq - off[e_out]
                    P, Q = (p, q) if o == 0 else (q, p)
                    assert P < self.d_start[v] and Q < self.d_end[v]
                    self.transit_count[self.transit_offsets[v] + P * self.d_end[v] + Q] += 1
                    self.totals[2] += 1
                    self.transit_segments.append((r, s))
        return self

    def matrix(self, u):
        o, ds, de = self.transit_offsets[u], self.d_start[u], self.d_end[u]
        return [self.transit_count[o + p * de:o + (p + 1) * de] for p in range(ds)]

    def judge(self, min_reads=1):
        """verdict and the summary words from the totals"""
        lim = max(min_reads, 1)
        self.verdict = []
        for u in range(self.n_unitigs):
            ds, de = self.d_start[u], self.d_end[u]
            if ds < 2 or de < 2:
                self.verdict.append(PLAIN)
                continue
            sup = [[c >= lim for c in row] for row in self.matrix(u)]
            rows, cols = [sum(row) for row in sup], [sum(sup[p][q] for p in range(ds)) for q in range(de)]
            if not any(rows):
                self.verdict.append(UNSPANNED)
            elif all(x == 1 for x in rows) and all(x == 1 for x in cols):
                assert ds == de
                self.verdict.append(RESOLVED)
            else:
                self.verdict.append(AMBIGUOUS)
        t = self.totals
        self.summary = [t[0], t[1], sum(1 for x in self.link_support if x == 0), t[2], t[3],
                        sum(1 for x in self.verdict if x != PLAIN), self.verdict.count(RESOLVED), self.verdict.count(AMBIGUOUS)]
        assert sum(self.transit_count) == t[2]
        return self

    def arrays(self):
        return self.link_support, self.transit_offsets, self.transit_count, self.verdict

    def text(self):
        """What the CLI's --transits prints."""
        off = self.lk.offsets
        out = ["L\t%d\t%d\t%d\n" % (e, self.lk.to[j], self.link_support[j])
               for e in range(len(off) - 1) for j in range(off[e], off[e + 1]) if self.link_support[j]]
        for u, v in enumerate(self.verdict):
            if v == PLAIN:
                continue
            out.append("U\t%d\t%s\t%d\t%d\n" % (u, VERDICT_NAMES[v], self.d_start[u], self.d_end[u]))
            out += ["T\t%d\t%d\t%d\t%d\n" % (u, p, q, c) for p, row in enumerate(self.matrix(u)) for q, c in enumerate(row) if c]
        return "".join(out)


def graph(table, canonical, min_count=1, max_count=0, k=None):
    """(unitig spellings, Links, k) of a table {k-mer string: count}; k is needed for an empty table only"""
    if not table:
        return [], lm.Links([0], [], 0, k), k
    u = um.unitigs(table, canonical, min_count, max_count)
    k = k if k is not None else len(next(iter(table)))
    return u.seqs, lm.links(table, canonical, min_count, max_count), k


def transits(table, canonical, batches, min_count=1, max_count=0, min_reads=1, k=None):
    """The model's Transits of a list of batches (each a list of read strings) accumulated on the graph of a table; .maps
    holds the map model of every batch"""
    seqs, lk, k = graph(table, canonical, min_count, max_count, k)
    t = Transits(lk, len(seqs), k)
    t.seqs, t.maps = seqs, []
    for reads in batches:
        m = mm.ReadMap(reads, k, canonical, seqs)
        t.add(m.read_segments)
        t.maps.append(m)
    return t.judge(min_reads)
