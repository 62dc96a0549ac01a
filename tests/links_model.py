"""The links between the unitigs of a count table's de Bruijn graph, restated with Python strings on top of graph_model.py
and unitig_model.py: the model the link tests compare kmc_unitig_links against.  It repeats the joins and the cycle cuts
of unitig_model.unitigs to know the terminal sides (they cannot be read off the spelled strings: a palindromic end key
would be ambiguous), walks the unitigs once more to name their two ends, and then applies the definition of include/kmc.h
literally.  brute_force() is independent of all that: it matches the spelled unitig strings by their (k-1)-overlaps."""
import graph_model as gm
import unitig_model as um

FIELDS = ("unitigs", "records", "ends_without", "ends_branching", "self_records", "dropped", "isolated_unitigs", "max_records")
_OTHER = {"R": "L", "L": "R"}


def cut_joins(table, canonical, min_count=1, max_count=0):
    """(keys in view order, solid set, joined after the cycle cuts): the first half of unitig_model.unitigs"""
    keys = sorted(table)
    row = {x: i for i, x in enumerate(keys)}
    solid = gm.solid_set(table, min_count, max_count)
    joined, _ = um.joins(canonical, solid)
    seen = set()
    for x in keys:
        if x not in solid or x in seen:
            continue
        path, cyc = um._walk(joined, x, "R")
        seen.add(x)
        seen.update(y for y, _ in path)
        if cyc:
            m = min([x] + [y for y, _ in path], key=row.get)
            b = joined.pop((m, "L"))
            if b != (m, "L"):
                joined.pop(b, None)
        else:
            seen.update(y for y, _ in um._walk(joined, x, "L")[0])
    return keys, solid, joined


def unitig_ends(keys, solid, joined, canonical):
    """{terminal side (key, side): end number 2u + e} with the unitigs numbered as unitig_model.unitigs numbers them"""
    row = {x: i for i, x in enumerate(keys)}
    found, seen = [], set()
    for x in keys:
        if x not in solid or x in seen:
            continue
        right, c1 = um._walk(joined, x, "R")
        left, c2 = um._walk(joined, x, "L")
        assert not c1 and not c2
        fwd = [(y, _OTHER[s]) for y, s in reversed(left)] + [(x, "R")] + right
        if canonical and row[fwd[-1][0]] < row[fwd[0][0]]:
            fwd = [(y, _OTHER[s]) for y, s in reversed(fwd)]
        seen.update(y for y, _ in fwd)
        found.append((row[fwd[0][0]], fwd))
    found.sort()
    end_of = {}
    for u, (_, fwd) in enumerate(found):
        start, end = (fwd[0][0], _OTHER[fwd[0][1]]), fwd[-1]    # the side opposite the first key's exit; the last key's exit
        assert start not in joined and end not in joined and start not in end_of and end not in end_of
        end_of[start] = 2 * u
        end_of[end] = 2 * u + 1
    terminals = {(x, s) for x in solid for s in "RL" if (x, s) not in joined}
    assert set(end_of) == terminals     # every terminal side of a solid key is exactly one unitig end
    return end_of


def summarize(offsets, to, dropped):
    n_ends = len(offsets) - 1
    per_end = [offsets[i + 1] - offsets[i] for i in range(n_ends)]
    return [n_ends // 2, len(to), sum(1 for m in per_end if m == 0), sum(1 for m in per_end if m >= 2),
            sum(1 for i in range(n_ends) for t in to[offsets[i]:offsets[i + 1]] if t >> 1 == i >> 1), dropped,
            sum(1 for u in range(n_ends // 2) if per_end[2 * u] == 0 and per_end[2 * u + 1] == 0), max(per_end, default=0)]


class Links:
    def __init__(self, offsets, to, dropped, k):
        self.offsets, self.to, self.k = offsets, to, k
        self.summary = summarize(offsets, to, dropped)

    def records(self):
        """(u, o1, v, o2) per record, in array order: leaving u through its END end reads u+, arriving at the START end of v
        reads v+"""
        for i in range(len(self.offsets) - 1):
            for t in self.to[self.offsets[i]:self.offsets[i + 1]]:
                yield i >> 1, "+" if i & 1 else "-", t >> 1, "-" if t & 1 else "+"


def links(table, canonical, min_count=1, max_count=0):
    keys, solid, joined = cut_joins(table, canonical, min_count, max_count)
    end_of = unitig_ends(keys, solid, joined, canonical)
    side_of = {e: a for a, e in end_of.items()}
    offsets, to, dropped = [0], [], 0
    for i in range(len(end_of)):
        x, s = side_of[i]
        for _, y, t in gm.neighbours(x, s, canonical, solid):   # ascending base code
            if (y, t) in joined:
                dropped += 1
            else:
                to.append(end_of[(y, t)])
        offsets.append(len(to))
    return Links(offsets, to, dropped, len(keys[0]) if keys else 0)


def brute_force(seqs, k, canonical):
    """The records from the spelled unitigs alone: end (u, o1) links to (v, o2) iff the last k - 1 bases of the oriented u
    equal the first k - 1 of the oriented v (both joined k-mers are k-mers of unitigs, so they are solid).  A forward ctx has
    one orientation.  Within an end the records are in ascending order of the base that extends the STORED end key, which
    the spelled strings determine as long as no key is its own reverse complement (forward ctx, or odd k)."""
    def orient(s, o):
        return s if o == "+" else gm.revcomp(s)

    offsets, to = [0], []
    for u, su in enumerate(seqs):
        for e in (0, 1):
            recs = []
            for v, sv in enumerate(seqs):
                if canonical:
                    a = orient(su, "+" if e else "-")            # leaving through the END end reads u+, through START u-
                    for o2 in "+-":
                        b = orient(sv, o2)
                        if a[len(a) - (k - 1):] != b[:k - 1]:
                            continue
                        last, nxt = a[-k:], b[k - 1]             # the stored end key is canon(last): read as it is, the
                        c = nxt if gm.canon(last, True) == last else gm.revcomp(nxt)   # base is appended; else prepended
                        recs.append((gm.BASES.index(c), 2 * v + (0 if o2 == "+" else 1)))
                elif e:                                          # forward, END end: whoever starts with its last k - 1
                    if su[len(su) - (k - 1):] == sv[:k - 1]:
                        recs.append((gm.BASES.index(sv[k - 1]), 2 * v))
                else:                                            # forward, START end: whoever ends in its first k - 1
                    if sv[len(sv) - (k - 1):] == su[:k - 1]:
                        recs.append((gm.BASES.index(sv[-k]), 2 * v + 1))
            recs.sort()
            to += [t for _, t in recs]
            offsets.append(len(to))
    return offsets, to


def gfa(unitigs, lk, k):
    """What the CLI's --gfa prints (unitigs: unitig_model.Unitigs, lk: Links)."""
    out = ["H\tVN:Z:1.0\n"]
    out += ["S\t%d\t%s\tLN:i:%d\tKC:i:%d\tCL:i:%d\n" % (i, s, len(s), a, f)
            for i, (s, a, f) in enumerate(zip(unitigs.seqs, unitigs.abund, unitigs.flags))]
    out += ["L\t%d\t%s\t%d\t%s\t%dM\n" % (u, o1, v, o2, k - 1) for u, o1, v, o2 in lk.records()]
    return "".join(out)
