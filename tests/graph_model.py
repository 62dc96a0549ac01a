"""The de Bruijn graph of a count table, restated with Python strings, a dict and a set: the model the graph tests compare
kmc_graph against.  It follows the definition of include/kmc.h in its NEIGHBOUR form -- a side continues iff its degree is
1 and the side of that one neighbour which faces back has degree 1 too -- and shares no code with the kernel, which uses
the equivalent sibling form (sibling_continues below restates that one, so that the equivalence itself is tested)."""

_COMP = str.maketrans("ACGT", "TGCA")
BASES = "ACGT"
END_R, END_L, SOLID = 1 << 8, 1 << 9, 1 << 10
FIELDS = ("nodes", "right_degrees", "left_degrees", "isolated", "dead_ends", "branching", "end_sides", "single_node_unitigs")


def revcomp(s):
    return s[::-1].translate(_COMP)


def canon(f, canonical):
    return min(f, revcomp(f)) if canonical else f


def solid_set(table, min_count=1, max_count=0):
    """table: {k-mer string: count}.  The keys with min_count <= count <= max_count (max_count 0: no upper bound)."""
    return {x for x, c in table.items() if c >= min_count and (max_count == 0 or c <= max_count)}


def extension(x, side, base, canonical):
    """(neighbour key, the side of it that faces x) of extending x on `side` ('R' / 'L') by `base`."""
    f = x[1:] + base if side == "R" else base + x[:-1]
    y = canon(f, canonical)
    kept = y == f
    if side == "R":
        return y, ("L" if kept else "R")
    return y, ("R" if kept else "L")


def neighbours(x, side, canonical, solid):
    """[(base code, neighbour, facing side)] over the bases whose extension is solid."""
    out = []
    for c, b in enumerate(BASES):
        y, facing = extension(x, side, b, canonical)
        if y in solid:
            out.append((c, y, facing))
    return out


def continues(x, side, canonical, solid):
    nb = neighbours(x, side, canonical, solid)
    if len(nb) != 1:
        return False
    _, y, facing = nb[0]
    return len(neighbours(y, facing, canonical, solid)) == 1


def sibling_continues(x, side, canonical, solid):
    """The form the kernel uses: degree 1 and exactly one of the four keys that share the overlap with x is solid."""
    if len(neighbours(x, side, canonical, solid)) != 1:
        return False
    if side == "R":
        sib = [canon(d + x[1:], canonical) for d in BASES]
    else:
        sib = [canon(x[:-1] + d, canonical) for d in BASES]
    return sum(1 for s in sib if s in solid) == 1


def adj_word(x, canonical, solid, cont=continues):
    if x not in solid:
        return 0
    a = SOLID
    for c, _, _ in neighbours(x, "R", canonical, solid):
        a |= 1 << c
    for c, _, _ in neighbours(x, "L", canonical, solid):
        a |= 16 << c
    if not cont(x, "R", canonical, solid):
        a |= END_R
    if not cont(x, "L", canonical, solid):
        a |= END_L
    return a


def summarize(adj):
    """The eight summary words from the adj words."""
    w = [0] * 8
    for a in adj:
        if not a & SOLID:
            continue
        dr, dl = bin(a & 15).count("1"), bin((a >> 4) & 15).count("1")
        er, el = (a >> 8) & 1, (a >> 9) & 1
        w[0] += 1
        w[1] += dr
        w[2] += dl
        w[3] += dr == 0 and dl == 0
        w[4] += (dr == 0) != (dl == 0)
        w[5] += dr >= 2 or dl >= 2
        w[6] += er + el
        w[7] += er & el
    return [int(v) for v in w]


def graph(table, canonical, min_count=1, max_count=0, cont=continues):
    """(keys in view order, adj words, summary words) of a table {k-mer string: count}."""
    keys = sorted(table)
    solid = solid_set(table, min_count, max_count)
    adj = [adj_word(x, canonical, solid, cont) for x in keys]
    return keys, adj, summarize(adj)


def graph_text(table, canonical, min_count=1, max_count=0):
    """What the CLI's --graph prints."""
    keys, adj, _ = graph(table, canonical, min_count, max_count)
    lines = []
    for x, a in zip(keys, adj):
        if not a & SOLID:
            continue
        r = "".join(b for c, b in enumerate(BASES) if (a >> c) & 1) or "."
        l = "".join(b for c, b in enumerate(BASES) if (a >> (4 + c)) & 1) or "."
        ends = ("L" if a & END_L else "") + ("R" if a & END_R else "") or "."
        lines.append("%s\t%d\t%s\t%s\t%s\n" % (x, table[x], r, l, ends))
    return "".join(lines)


def stats_text(words):
    """What the CLI's --graph-stats prints."""
    return "".join("%s\t%d\n" % (f, w) for f, w in zip(FIELDS, words)) + "unitigs\t%d\n" % (words[6] // 2)


def count_table(reads, k, canonical):
    """{k-mer: count} of a list of read strings, windows with a character outside ACGT skipped."""
    t = {}
    for s in reads:
        for j in range(len(s) - k + 1):
            w = s[j:j + k]
            if w.strip("ACGT"):   # something is left when the ACGT characters at both ends are stripped
                continue
            key = canon(w, canonical)
            t[key] = t.get(key, 0) + 1
    return t
