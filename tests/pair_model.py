"""Pair evidence restated over Python lists: the model the pairs tests compare kmc_unitig_pairs against.  It takes the
segments of map_model.ReadMap and the unitig spellings of unitig_model.unitigs and follows the definitions of include/kmc.h
literally -- anchor, out end, reach, class, record.  KMC_PAIR_ACCUMULATE is modelled as concatenation: the batches are laid
end to end and the per-pair arrays of the last one cut off.  It shares no code with the library."""
import map_model as mm
import unitig_model as um

NONE = 0xFFFFFFFF
UNPLACED, SPAN, PROPER, EVERTED, SAME_STRAND = 0, 1, 2, 3, 4
FIELDS = ("pairs", "unplaced", "span", "proper", "everted", "same_strand", "records", "insert_sum")


def anchor(segs):
    """the longest segment of a read, of equally long ones the last; None without a segment"""
    best = None
    for s in segs:
        if best is None or s[1] >= best[1]:
            best = s
    return best


def end_and_reach(seg, k, seqs):
    """(e, u, reach) of an anchor (start, len, uni, pos)"""
    start, _, uni, pos = seg
    u, o = uni >> 1, uni & 1
    m = len(seqs[u]) - k + 1
    assert 0 <= pos < m
    return 2 * u + 1 - o, u, start + (pos + 1 if o else m - pos) + k - 1


class Pairs:
    def __init__(self, batches, k, canonical, seqs, n_bins):
        """batches: lists of read strings, mates adjacent; the per-pair arrays are those of the last batch"""
        self.k, self.n_bins, self.seqs = k, n_bins, seqs
        self.maps = [mm.ReadMap(b, k, canonical, seqs) for b in batches]
        recs, self.hist, self.summary = {}, [0] * n_bins, [0] * 8
        self.ties = 0                       # mates whose anchor had an equally long rival
        for m in self.maps:
            assert len(m.read_segments) % 2 == 0
            self.pair_class, self.pair_ends, self.pair_value = [], [], []
            for i in range(len(m.read_segments) // 2):
                a, b = anchor(m.read_segments[2 * i]), anchor(m.read_segments[2 * i + 1])
                for segs, x in ((m.read_segments[2 * i], a), (m.read_segments[2 * i + 1], b)):
                    if x is not None and sum(1 for s in segs if s[1] == x[1]) > 1:
                        self.ties += 1
                        assert x == [s for s in segs if s[1] == x[1]][-1]
                cls, ends, val = UNPLACED, [NONE if a is None else end_and_reach(a, k, seqs)[0], NONE if b is None else end_and_reach(b, k, seqs)[0]], 0
                if a is not None and b is not None:
                    (ea, ua, ra), (eb, ub, rb) = end_and_reach(a, k, seqs), end_and_reach(b, k, seqs)
                    R = ra + rb
                    if ua != ub:
                        cls, val = SPAN, R
                        r = recs.setdefault((min(ea, eb), max(ea, eb)), [0, 0, R, R])
                        r[0] += 1; r[1] += R; r[2] = min(r[2], R); r[3] = max(r[3], R)
                    elif (a[2] & 1) != (b[2] & 1):
                        L = len(seqs[ua])
                        if R > L:
                            cls, val = PROPER, R - L
                            self.hist[min(val, n_bins - 1)] += 1
                            self.summary[7] += val
                        else:
                            cls = EVERTED
                    else:
                        cls = SAME_STRAND
                self.pair_class.append(cls); self.pair_ends.append(ends); self.pair_value.append(val)
                self.summary[0] += 1
                self.summary[1 + cls] += 1
        if not self.maps:
            self.pair_class, self.pair_ends, self.pair_value = [], [], []
        keys = sorted(recs)
        self.rec_ends = [list(x) for x in keys]
        self.rec_count, self.rec_sum, self.rec_min, self.rec_max = ([recs[x][j] for x in keys] for j in range(4))
        self.summary[6] = len(keys)
        s = self.summary
        assert s[0] == sum(s[1:6]) and sum(self.rec_count) == s[2] and sum(self.hist) == s[3] and s[6] <= s[2] and self.hist[0] == 0

    def arrays(self):
        return (self.pair_class, self.pair_ends, self.pair_value, self.rec_ends, self.rec_count, self.rec_sum, self.rec_min, self.rec_max, self.hist)

    def totals(self):
        """what is additive: everything but the per-pair arrays"""
        return self.arrays()[3:] + (self.summary,)

    def text(self):
        """What the CLI's --pairs prints."""
        out = ["I\t%d\t%d\n" % (f, n) for f, n in enumerate(self.hist) if n]
        out += ["P\t%d\t%d\t%d\t%d\t%d\t%d\n" % (a, b, c, s, lo, hi)
                for (a, b), c, s, lo, hi in zip(self.rec_ends, self.rec_count, self.rec_sum, self.rec_min, self.rec_max)]
        return "".join(out)


def pairs(table, canonical, batches, min_count=1, max_count=0, n_bins=1024, k=None):
    """The model's Pairs of a list of batches (each a list of read strings, mates adjacent) on the unitigs of a table
    {k-mer string: count}; k is needed for an empty table only."""
    u = um.unitigs(table, canonical, min_count, max_count)
    k = k if k is not None else len(next(iter(table)))
    return Pairs(batches, k, canonical, u.seqs, n_bins)
