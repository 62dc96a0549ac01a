"""The connected components of the compacted graph, restated with Python integers on top of unitig_model.unitigs and
links_model.links: the model the components tests compare kmc_unitig_components against.  components_from is the definition
of include/kmc.h on plain lists (keys per unitig, abundances, link offsets and targets): a union-find over the records,
components numbered by their smallest unitig.  brute_force is independent of the unitigs' links: a breadth-first search
over the solid KEYS with graph_model.neighbours, mapped to unitigs afterwards.  np_components is the numpy form the measure
tool times as the host baseline."""
import numpy as np

import graph_model as gm
import links_model as lm
import unitig_model as um

FIELDS = ("unitigs", "components", "single_unitig", "max_keys", "max_unitigs", "small", "kept_keys", "kept_count")
KEEP, COMPONENT = 0, 4
UNLIMITED = 1 << 31


def _small(keys, limit):
    return limit != 0 and (limit >= UNLIMITED or keys <= limit)


def components_from(m, abund, offsets, to, limit):
    """(comp_of per unitig, [root, unitigs, keys, abund] per component, verdict per unitig) from m[u] keys, abund[u] and the
    records to[offsets[e]:offsets[e + 1]] of end e"""
    nu = len(m)
    parent = list(range(nu))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for e in range(2 * nu):
        for t in to[offsets[e]:offsets[e + 1]]:
            a, b = find(e >> 1), find(t >> 1)
            if a != b:
                parent[max(a, b)] = min(a, b)
    roots = [u for u in range(nu) if find(u) == u]           # ascending, and a root is the smallest id of its class
    number = {r: c for c, r in enumerate(roots)}
    comp_of = [number[find(u)] for u in range(nu)]
    stats = [[r, 0, 0, 0] for r in roots]
    for u, c in enumerate(comp_of):
        assert stats[c][0] <= u
        stats[c][1] += 1
        stats[c][2] += m[u]
        stats[c][3] += abund[u]
    verdict = [COMPONENT if _small(stats[c][2], limit) else KEEP for c in comp_of]
    return comp_of, stats, verdict


class Components:
    def __init__(self, comp_of, stats, verdict, kept, summary, unitigs, links):
        self.comp_of, self.stats, self.verdict, self.kept, self.summary = comp_of, stats, verdict, kept, summary
        self.unitigs, self.links = unitigs, links

    @property
    def removed(self):
        return self.summary[5]

    def members(self, c):
        return [u for u, x in enumerate(self.comp_of) if x == c]

    def text(self):
        """What the CLI's --components prints."""
        return "".join("%d\t%d\t%d\t%d\t%d\n" % (c, s[0], s[1], s[2], s[3]) for c, s in enumerate(self.stats))


def components(table, canonical, min_count=1, max_count=0, limit=0, graph=None):
    """The components, the verdicts, the kept {k-mer: count} and the summary words of a table {k-mer string: count}.
    graph: (unitig_model.unitigs, links_model.links) of this table and range, if the caller has them already."""
    u, lk = graph or (um.unitigs(table, canonical, min_count, max_count), lm.links(table, canonical, min_count, max_count))
    k = len(next(iter(table))) if table else 0
    m = [len(s) - k + 1 for s in u.seqs]
    comp_of, stats, verdict = components_from(m, u.abund, lk.offsets, lk.to, limit)
    kept = {}
    for s, v in zip(u.seqs, verdict):
        if v == KEEP:
            for j in range(len(s) - k + 1):
                x = gm.canon(s[j:j + k], canonical)
                kept[x] = table[x]
    small = [s for s in stats if _small(s[2], limit)]
    assert len(kept) + sum(s[2] for s in small) == u.summary[2]
    summary = [len(m), len(stats), sum(1 for s in stats if s[1] == 1), max((s[2] for s in stats), default=0),
               max((s[1] for s in stats), default=0), len(small), len(kept), sum(kept.values())]
    return Components(comp_of, stats, verdict, kept, summary, u, lk)


def rounds(table, canonical, min_count=1, max_count=0, limit=0, n_rounds=1):
    """(the table after the rounds, [the summary of every round run]): a round drops the small components of the table of
    the round before with the same range and limit; the loop stops after a round that removes nothing."""
    out = []
    for _ in range(n_rounds):
        c = components(table, canonical, min_count, max_count, limit)
        out.append(c.summary)
        table = c.kept
        if c.removed == 0:
            break
    return table, out


def brute_force(table, canonical, min_count=1, max_count=0):
    """comp_of per unitig of unitig_model.unitigs, from the KEYS alone: a breadth-first search over the solid keys along
    graph_model.neighbours on both sides, every class of keys then mapped to the unitigs that hold its keys, the classes
    numbered by their smallest unitig.  Valid where no key is its own reverse complement (a forward ctx, or odd k): only
    there is the neighbour relation symmetric and no record dropped -- the caveat of links_model.brute_force."""
    solid = gm.solid_set(table, min_count, max_count)
    u = um.unitigs(table, canonical, min_count, max_count)
    k = len(next(iter(table))) if table else 0
    unitig_of = {}
    for i, s in enumerate(u.seqs):
        for j in range(len(s) - k + 1):
            unitig_of[gm.canon(s[j:j + k], canonical)] = i
    assert set(unitig_of) == solid
    label, classes = {}, []
    for x in sorted(solid):
        if x in label:
            continue
        label[x] = len(classes)
        todo, seen = [x], {unitig_of[x]}
        while todo:
            y = todo.pop()
            for side in "RL":
                for _, z, _ in gm.neighbours(y, side, canonical, solid):
                    if z not in label:
                        label[z] = len(classes)
                        seen.add(unitig_of[z])
                        todo.append(z)
        classes.append(seen)
    # a unitig's keys are one path, so every unitig lies in exactly one class
    assert sum(len(c) for c in classes) == len(u.seqs)
    order = sorted(range(len(classes)), key=lambda c: min(classes[c]))
    comp_of = [0] * len(u.seqs)
    for number, c in enumerate(order):
        for i in classes[c]:
            comp_of[i] = number
    return comp_of


def np_components(offsets, to, m, abund, limit=0):
    """(comp_of uint32, stats uint64[n, 4], verdict uint8) from numpy arrays: link_offsets uint64[2 nu + 1], link_to uint32,
    keys and abundances per unitig.  Min-label hooking with pointer jumping, whole arrays per step."""
    nu = len(m)
    offsets = np.asarray(offsets, np.int64)
    src = np.repeat(np.arange(2 * nu, dtype=np.int64), np.diff(offsets)) >> 1
    dst = np.asarray(to, np.int64) >> 1
    parent = np.arange(nu, dtype=np.int64)
    for _ in range(nu + 1):
        a, b = parent[src], parent[dst]
        diff = a != b
        if not diff.any():
            break
        np.minimum.at(parent, np.maximum(a, b)[diff], np.minimum(a, b)[diff])
        for _ in range(64):
            nxt = parent[parent]
            if np.array_equal(nxt, parent):
                break
            parent = nxt
    is_root = parent == np.arange(nu)
    rank = np.cumsum(is_root) - 1
    comp_of = rank[parent] if nu else np.zeros(0, np.int64)
    nc = int(is_root.sum())
    stats = np.zeros((nc, 4), np.uint64)
    stats[:, 0] = np.flatnonzero(is_root)
    stats[:, 1] = np.bincount(comp_of, minlength=nc)
    for col, val in ((2, m), (3, abund)):
        acc = np.zeros(nc, np.uint64)
        np.add.at(acc, comp_of, np.asarray(val, np.uint64))
        stats[:, col] = acc
    small = np.zeros(nc, bool) if limit == 0 else (np.ones(nc, bool) if limit >= UNLIMITED else stats[:, 2] <= np.uint64(limit))
    verdict = np.where(small[comp_of], COMPONENT, KEEP).astype(np.uint8) if nu else np.zeros(0, np.uint8)
    return comp_of.astype(np.uint32), stats, verdict
