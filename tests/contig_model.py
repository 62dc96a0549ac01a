"""Contigs from the counted read walks, restated in plain Python on top of transit_model.Transits (support per link record,
transit counts per unitig) and unitig_model.py (spellings, abundances): the model the contig tests compare
kmc_unitig_contigs against.  It follows the definition of include/kmc.h literally -- RESOLVED, NODE, CHOICE, JOIN, CONTIG --
over Python lists, by WALKING from node to node, and shares no code with the library, which ranks the node ends by pointer
doubling."""
import graph_model as gm
import transit_model as tm
import unitig_model as um

FIELDS = ("contigs", "nodes", "unitigs_duplicated", "records_ignored", "circular", "one_node", "most_nodes", "bases")
START, END = 0, 1


def sigma_of(t, u, min_reads):
    """sigma_u as a list (row P -> column Q) if unitig u is RESOLVED under min_reads, else None"""
    ds, de = t.d_start[u], t.d_end[u]
    if ds < 2 or de < 2:
        return None
    lim = max(min_reads, 1)
    sup = [[c >= lim for c in row] for row in t.matrix(u)]
    if not all(sum(row) == 1 for row in sup) or not all(sum(sup[p][q] for p in range(ds)) == 1 for q in range(de)):
        return None
    assert ds == de
    return [row.index(True) for row in sup]


class Contigs:
    def __init__(self, t, unitigs, min_reads=1, min_support=0):
        """t: transit_model.Transits of the graph, unitigs: unitig_model.Unitigs of the same table and range"""
        self.t, self.k = t, t.k
        k, off, to = t.k, t.lk.offsets, t.lk.to
        nu = t.n_unitigs
        assert nu == len(unitigs.seqs)
        sigma = [sigma_of(t, u, min_reads) for u in range(nu)]
        copies = [len(s) if s is not None else 1 for s in sigma]
        self.node_offsets = [0]
        for c in copies:
            self.node_offsets.append(self.node_offsets[-1] + c)
        n_nodes = self.node_offsets[-1]
        owner = [(u, p) for u in range(nu) for p in range(copies[u])]
        ignored = 0
        if min_support:
            for u in range(nu):
                if sigma[u] is None:
                    ignored += sum(1 for j in range(off[2 * u], off[2 * u + 2]) if t.link_support[j] < min_support)

        def choice(n, e):
            u, p = owner[n]
            s = 2 * u + e
            if sigma[u] is not None:
                j = off[s] + (p if e == START else sigma[u][p])
            else:
                live = [j for j in range(off[s], off[s + 1]) if not min_support or t.link_support[j] >= min_support]
                if len(live) != 1:
                    return None
                j = live[0]
            w, f = to[j] >> 1, to[j] & 1
            if sigma[w] is None:
                return self.node_offsets[w], f
            back = to[off[to[j]]:off[to[j] + 1]]
            if s not in back:
                return None
            q = back.index(s)
            return self.node_offsets[w] + (q if f == START else sigma[w].index(q)), f

        ch = {(n, e): choice(n, e) for n in range(n_nodes) for e in (START, END)}
        joined = {a: b for a, b in ch.items() if b is not None and b != a and ch[b] == a}
        # cycles: cut at the join of the START end of the smallest node
        seen, circular = set(), set()
        for n in range(n_nodes):
            if n in seen:
                continue
            comp, cur, cyc = [n], (n, END), False
            while cur in joined:          # leave through END and go on
                m, f = joined[cur]
                if m == n:
                    cyc = True
                    break
                comp.append(m)
                cur = (m, 1 - f)
            if not cyc:
                cur = (n, START)
                while cur in joined:
                    m, f = joined[cur]
                    comp.append(m)
                    cur = (m, 1 - f)
            seen.update(comp)
            if cyc:
                m = min(comp)
                b = joined.pop((m, START))
                joined.pop(b)
                circular.add(m)
        # paths: from the end node with the smaller id
        found, seen = [], set()
        for n in range(n_nodes):
            if n in seen:
                continue

            def walk(first, enter):
                """the nodes from `first`, entered through end `enter`, as (node, o); o = 1: entered through END, read reversed"""
                out, cur = [], (first, enter)
                while True:
                    out.append((cur[0], cur[1]))
                    nxt = (cur[0], 1 - cur[1])
                    if nxt not in joined:
                        return out
                    cur = joined[nxt]

            # the two end nodes of n's path
            back = walk(n, END)[-1]       # walking out through START ends at this node, whose far end is unjoined
            fwd = walk(n, START)[-1]
            e1, e2 = (back[0], 1 - back[1]), (fwd[0], 1 - fwd[1])     # the unjoined node ends
            if e1[0] == e2[0]:
                start = (e1[0], START)                                  # one node: read +
                assert e1[0] == n and (n, START) not in joined and (n, END) not in joined
            else:
                start = e1 if e1[0] < e2[0] else e2
            nodes = walk(*start)
            assert not seen & {m for m, _ in nodes} and len({m for m, _ in nodes}) == len(nodes)
            seen.update(m for m, _ in nodes)
            found.append((nodes[0][0], nodes))
        found.sort()
        self.path_offsets, self.path, self.seqs, self.abund, self.flags = [0], [], [], [], []
        for first, nodes in found:
            entries = [2 * owner[m][0] + o for m, o in nodes]
            spelled = [unitigs.seqs[x >> 1] if not x & 1 else gm.revcomp(unitigs.seqs[x >> 1]) for x in entries]
            self.path += entries
            self.path_offsets.append(len(self.path))
            self.seqs.append(spelled[0] + "".join(s[k - 1:] for s in spelled[1:]))
            self.abund.append(sum(unitigs.abund[x >> 1] for x in entries))
            self.flags.append(1 if first in circular else 0)
        self.spelled_overlaps_agree = all(
            (unitigs.seqs[a >> 1] if not a & 1 else gm.revcomp(unitigs.seqs[a >> 1]))[-(k - 1):] ==
            (unitigs.seqs[b >> 1] if not b & 1 else gm.revcomp(unitigs.seqs[b >> 1]))[:k - 1]
            for c in range(len(self.seqs)) for a, b in zip(self.path[self.path_offsets[c]:self.path_offsets[c + 1] - 1],
                                                           self.path[self.path_offsets[c] + 1:self.path_offsets[c + 1]])) if k > 1 else True
        self.copies = copies
        self.bases = "".join(self.seqs)
        self.offsets = [0]
        for s in self.seqs:
            self.offsets.append(self.offsets[-1] + len(s))
        sizes = [self.path_offsets[c + 1] - self.path_offsets[c] for c in range(len(self.seqs))]
        self.summary = [len(self.seqs), n_nodes, sum(1 for s in sigma if s is not None), ignored, sum(self.flags),
                        sum(1 for x in sizes if x == 1), max(sizes, default=0), len(self.bases)]

    def paths(self):
        return [self.path[self.path_offsets[c]:self.path_offsets[c + 1]] for c in range(len(self.seqs))]

    def walks(self):
        return ["".join("%s%d" % ("<" if e & 1 else ">", e >> 1) for e in p) for p in self.paths()]

    def text(self):
        """What the CLI's --contigs prints."""
        return "".join(">%d LN:i:%d KC:i:%d CL:i:%d WK:Z:%s\n%s\n" % (i, len(s), a, f, w, s)
                       for i, (s, a, f, w) in enumerate(zip(self.seqs, self.abund, self.flags, self.walks())))


def contigs(table, canonical, batches, min_count=1, max_count=0, min_reads=1, min_support=0, k=None):
    """The model's Contigs of a table {k-mer string: count} under the reads of `batches` (lists of strings, accumulated)"""
    t = tm.transits(table, canonical, batches, min_count, max_count, min_reads, k)
    u = um.unitigs(table, canonical, min_count, max_count)
    return Contigs(t, u, min_reads, min_support)
