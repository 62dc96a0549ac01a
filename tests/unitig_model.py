"""The unitigs of a count table's de Bruijn graph, restated with Python strings on top of graph_model.py: the model the
unitig tests compare kmc_unitigs against.  It follows the definition of include/kmc.h literally -- partner, mutual join,
cut of a cycle at side L of its smallest row, start at the end key of the smaller row -- by WALKING from key to key, and
shares no code with the kernels, which rank the side states by pointer doubling."""
import graph_model as gm

FIELDS = ("unitigs", "bases", "keys", "circular", "one_key", "longest_keys", "unjoined_sides", "abundance")
_OTHER = {"R": "L", "L": "R"}


def joins(canonical, solid):
    """({side: the side it is joined to}, the number of sides that continue and are not joined).  partner(a) = (y, T), the
    one solid neighbour on a side that continues (graph_model.continues, with every side's neighbours listed once) and the
    side of it that faces back."""
    nb = {(x, s): [(y, t) for _, y, t in gm.neighbours(x, s, canonical, solid)] for x in solid for s in "RL"}
    part = {a: v[0] for a, v in nb.items() if len(v) == 1 and len(nb[v[0]]) == 1}
    joined, lost = {}, 0
    for a, b in part.items():
        if b != a and part.get(b) == a:
            joined[a] = b
        else:
            lost += 1
    return joined, lost


def _walk(joined, x, side):
    """Leave x through `side` and go on until a terminal: [(key, the side it is left through)], and whether the walk came
    back to x (a cycle)."""
    out, cur = [], (x, side)
    while cur in joined:
        y, t = joined[cur]
        if y == x:
            return out, True
        cur = (y, _OTHER[t])
        out.append(cur)
    return out, False


class Unitigs:
    def __init__(self, seqs, abund, flags, lost, k):
        self.seqs, self.abund, self.flags = seqs, abund, flags
        self.bases = "".join(seqs)
        self.offsets = [0]
        for s in seqs:
            self.offsets.append(self.offsets[-1] + len(s))
        keys = [len(s) - k + 1 for s in seqs]
        self.summary = [len(seqs), len(self.bases), sum(keys), sum(flags), sum(1 for m in keys if m == 1), max(keys, default=0), lost,
                        sum(abund)]

    def fasta(self):
        """What the CLI's --unitigs prints."""
        return "".join(">%d LN:i:%d KC:i:%d CL:i:%d\n%s\n" % (i, len(s), a, f, s) for i, (s, a, f) in enumerate(zip(self.seqs, self.abund, self.flags)))


def unitigs(table, canonical, min_count=1, max_count=0):
    """The unitigs of a table {k-mer string: count}, in order."""
    keys = sorted(table)
    row = {x: i for i, x in enumerate(keys)}
    k = len(keys[0]) if keys else 0
    solid = gm.solid_set(table, min_count, max_count)
    joined, lost = joins(canonical, solid)
    # cycles: cut on the L side of the smallest row
    seen, circular = set(), set()
    for x in keys:
        if x not in solid or x in seen:
            continue
        path, cyc = _walk(joined, x, "R")
        seen.add(x)
        seen.update(y for y, _ in path)
        if cyc:
            m = min([x] + [y for y, _ in path], key=row.get)
            b = joined.pop((m, "L"))
            if b != (m, "L"):
                joined.pop(b, None)
            circular.add(m)
        else:
            seen.update(y for y, _ in _walk(joined, x, "L")[0])
    found, seen = [], set()
    for x in keys:
        if x not in solid or x in seen:
            continue
        right, c1 = _walk(joined, x, "R")
        left, c2 = _walk(joined, x, "L")
        assert not c1 and not c2
        # the direction that leaves x through R: from the end on its L side to the end on its R side
        fwd = [(y, _OTHER[s]) for y, s in reversed(left)] + [(x, "R")] + right
        e_l, e_r = fwd[0][0], fwd[-1][0]
        if canonical and row[e_r] < row[e_l]:
            fwd = [(y, _OTHER[s]) for y, s in reversed(fwd)]
        assert not seen & {y for y, _ in fwd} and len({y for y, _ in fwd}) == len(fwd)
        seen.update(y for y, _ in fwd)
        read = [y if s == "R" else gm.revcomp(y) for y, s in fwd]
        seq = read[0] + "".join(r[-1] for r in read[1:])
        found.append((row[fwd[0][0]], seq, sum(table[y] for y, _ in fwd), 1 if fwd[0][0] in circular else 0))
    found.sort()
    return Unitigs([f[1] for f in found], [f[2] for f in found], [f[3] for f in found], lost, k)


def kmers_of(u, k, canonical):
    """The keys of the unitigs' k-mers, in order of appearance."""
    return [gm.canon(s[j:j + k], canonical) for s in u.seqs for j in range(len(s) - k + 1)]
