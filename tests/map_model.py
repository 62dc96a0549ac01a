"""Reads threaded through the unitigs of a count table, restated with Python strings: the model the map tests compare
kmc_unitig_map against.  It takes the unitig spellings of unitig_model.unitigs, cuts every S_u into its m_u windows to build
a dictionary from key string to (u, pos), and then follows the definitions of include/kmc.h literally -- canon, dictionary
lookup, orientation by string comparison, segments by the CONTINUES formula.  It shares no code with the library."""
import graph_model as gm
import unitig_model as um

NONE = 0xFFFFFFFF
FIELDS = ("reads", "valid_windows", "placed_windows", "segments", "crossings", "reads_fully_placed", "reads_unplaced", "max_segments")
_ACGT = set("ACGT")


def key_places(seqs, k, canonical):
    """{key string: (u, pos)} over the windows of the unitig spellings"""
    where = {}
    for u, s in enumerate(seqs):
        for pos in range(len(s) - k + 1):
            x = gm.canon(s[pos:pos + k], canonical)
            assert x not in where, (x, where[x], (u, pos))     # a solid key occurs in exactly one unitig, once
            where[x] = (u, pos)
    return where


def place_read(read, k, canonical, where, seqs):
    """[(valid, uni, pos)] per base position of one read: uni = 2u + o or NONE"""
    out = []
    for j in range(len(read)):
        f = read[j:j + k]
        if len(f) < k or not set(f) <= _ACGT:
            out.append((False, NONE, 0))
            continue
        hit = where.get(gm.canon(f, canonical))
        if hit is None:
            out.append((True, NONE, 0))
            continue
        u, pos = hit
        o = 0 if seqs[u][pos:pos + k] == f else 1
        assert o == 0 or (canonical and seqs[u][pos:pos + k] == gm.revcomp(f))
        out.append((True, 2 * u + o, pos))
    return out


def continues(a, b):
    """window b (valid, uni, pos) continues its predecessor a"""
    if a[1] == NONE or b[1] == NONE or a[1] != b[1]:
        return False
    return b[2] == a[2] + 1 if b[1] % 2 == 0 else b[2] == a[2] - 1


def segments_of(placed):
    """([(start, len, uni, pos)], crossings) of one read's placements"""
    segs, crossings = [], 0
    for j, w in enumerate(placed):
        if w[1] == NONE:
            continue
        if j > 0 and continues(placed[j - 1], w):
            s = segs[-1]
            segs[-1] = (s[0], s[1] + 1, s[2], s[3])
            continue
        segs.append((j, 1, w[1], w[2]))
        if j > 0 and placed[j - 1][1] != NONE:
            crossings += 1
    return segs, crossings


class ReadMap:
    def __init__(self, reads, k, canonical, seqs):
        where = key_places(seqs, k, canonical)
        self.k, self.n_unitigs = k, len(seqs)
        self.place, self.stats, self.seg_offsets, self.segments = [], [], [0], []
        self.support = [0] * len(seqs)
        self.read_segments = []
        for read in reads:
            placed = place_read(read, k, canonical, where, seqs)
            segs, crossings = segments_of(placed)
            self.place += [(pos << 32) | uni for _, uni, pos in placed]
            n_valid, n_placed = sum(1 for w in placed if w[0]), sum(1 for w in placed if w[1] != NONE)
            assert n_placed == sum(s[1] for s in segs)
            self.stats.append([n_valid, n_placed, len(segs), crossings])
            self.segments += segs
            self.read_segments.append(segs)
            self.seg_offsets.append(len(self.segments))
            for _, uni, _ in placed:
                if uni != NONE:
                    self.support[uni >> 1] += 1
        st = self.stats
        self.summary = [len(reads), sum(s[0] for s in st), sum(s[1] for s in st), len(self.segments), sum(s[3] for s in st),
                        sum(1 for s in st if s[0] and s[1] == s[0]), sum(1 for s in st if s[1] == 0), max([s[2] for s in st], default=0)]

    def walks(self):
        """per read the stretches of KmerCounter.map_reads(...).walks()"""
        out = []
        for segs in self.read_segments:
            stretches, end = [], None
            for start, ln, uni, pos in segs:
                if end is None or start != end:
                    stretches.append([])
                stretches[-1].append((uni >> 1, uni & 1, pos, ln))
                end = start + ln
            out.append(stretches)
        return out

    def text(self):
        """What the CLI's --map prints."""
        lines = []
        for r, segs in enumerate(self.read_segments):
            walk, end = "", None
            for start, ln, uni, pos in segs:
                if end is not None and start != end:
                    walk += ","
                walk += "%s%d:%d:%d" % ("<" if uni & 1 else ">", uni >> 1, pos, ln)
                end = start + ln
            lines.append("%d\t%d\t%d\t%d\t%s\n" % (r, self.stats[r][0], self.stats[r][1], len(segs), walk or "*"))
        return "".join(lines)


def map_reads(table, canonical, reads, min_count=1, max_count=0, k=None):
    """The model's ReadMap of a list of read strings on the unitigs of a table {k-mer string: count}; k is needed for an
    empty table only."""
    u = um.unitigs(table, canonical, min_count, max_count)
    k = k if k is not None else len(next(iter(table)))
    return ReadMap(reads, k, canonical, u.seqs)
