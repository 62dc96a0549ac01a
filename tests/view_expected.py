"""The menu of tables, read batches and arguments of the view-sequence tests, and the expected result of every family for
every entry of it, from the models the per-family tests use (no GPU, no library):

  graph_model, unitig_model, links_model, map_model, transit_model, correct_model, trim_model, normalize_model, clean_model,
  bubble_model, bubble_call_model, components_model, setops_np; the table itself for export, filter, histogram and query
  (tests/test_view_sequences_host.py holds it against the CPU oracle's); normalize_model.window_counts for profile.

A table is named ("few" | "mid" | "big" | "empty", multiplicity): the reads counted once or twice.  A table a *_into step
leaves in the partner ctx is named ("kept", source table, family arguments).  Expected values are memoised per (table,
family, arguments): a result is an ordered dict {array name: numpy array}, the summary words last as "words", and the test
compares it byte for byte with what the library returns."""
import importlib
from collections import OrderedDict

import numpy as np

import bubble_call_model as bcm
import bubble_inputs as bi
import bubble_model as bm
import chunk_inputs
import clean_inputs as ci
import clean_model as cm
import components_model as pm
import correct_model as crm
import graph_model as gm
import links_model as lm
import map_inputs as mi
import map_model as mm
import normalize_model as nm
import setops_np as so
import transit_inputs as ti
import transit_model as tm
import trim_model as trm
import unitig_model as um

U64, U32, U16, U8 = np.uint64, np.uint32, np.uint16, np.uint8
M64 = (1 << 64) - 1

CONFIGS = ((31, True), (32, True), (33, False))
RANGES = ((1, 0), (2, 0), (2, 40))
N_PARTS = 3
HIST_BINS = 8
TRIM_RULES = (    # (mode, flags, min_strong, min_permille, min_len): the modes and flags of the header's table
    (trm.LONGEST, 0, 0, 0, 0), (trm.ENDS, 0, 1, 500, 20), (trm.NONE, trm.INVERT, 1, 0, 0), (trm.NONE, trm.PAIR_BOTH, 1, 0, 0),
    (trm.LONGEST, trm.PAIR_EITHER, 0, 0, 40))
NORM_RULES = (    # (permille, target, min_depth, seed, flags)
    (500, 0, 0, 0, 0), (500, 2, 1, 7, 0), (0, 1, 0, 3, nm.PAIRED), (1000, 3, 2, 11, nm.INVERT))
SETOPS = (("compare",), ("setop", so.INTERSECT, so.MIN), ("setop", so.UNION, so.SUM), ("setop", so.SUBTRACT, so.LEFT), ("setop", so.UNION, so.DIFF))
INTO_KINDS = ("clean", "simplify", "components")


def clean_limits(k):
    return ((k, k), (4, 0))


def simplify_limits(k):
    return ((k, k, k), (k, k, 0))       # the second shares its result with clean (k, k)


def component_limits(k):
    return ((k,), (3,))


def bubble_limits(k):
    return ((k,), (2 * k,))


def _rnd(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def few_reads(k, seed):
    """the "few" shapes of test_unitig_gpu.py (short reads, a fork, a homopolymer, an AT repeat, circular reads, for even k
    a palindrome) and two more short reads: about sixty keys"""
    from test_unitig_gpu import _constructed
    rng = np.random.default_rng(seed + 1)
    return _constructed(k, seed, few=True) + [_rnd(rng, k + 9), _rnd(rng, k + 7)]


def mid_reads(k, seed):
    """a few hundred keys: a fork with a tip (clean_inputs), an island, a simple bubble (bubble_inputs.substitution), a
    circular unitig and a one-key cycle (map_inputs.circular), a 2 x 2 repeat (transit_inputs.repeat), for even k a
    palindromic key"""
    rng = np.random.default_rng([seed, 3])      # (the builders seed generators of their own: every one gets another stream)
    reads = ci.fork(rng, 2 * k + 5, (4, 4), (2, 1))[0] + [ci.rnd(rng, k + 2)] + bi.substitution(k, seed + 1)[0]
    reads += mi.circular(k, seed + 2, 20)[0] + ti.repeat(k, seed)[0]
    if k % 2 == 0:
        half = _rnd(rng, k // 2)
        reads.append("G" + half + gm.revcomp(half) + "C")
    return reads


def big_reads(k, seed, canonical=True):
    """between 2049 and 2600 keys, three tiles of the 1024-row scans: the mid table's shapes with other seeds, a genome of
    1700 keys read once, its first 700 bases read again and a stretch of it once more (on the other strand where that
    adds no keys)"""
    rng = np.random.default_rng(seed + 7)
    g = _rnd(rng, 1700 + k - 1)
    return mid_reads(k, seed + 100) + [g, g[:700], gm.revcomp(g[300:900]) if canonical else g[300:900]]


def batch_a(k, seed, canonical=True):
    """forty reads of 0 to 300 bases cut from the mid and big samples (so they cross unitig ends: forks, the bubble, the
    repeat, the cycle) on either strand, some with a substituted base, an N or a lower-case letter; an empty read; one
    read longer than one chunk of the shared window front end; the reads that span the repeat of the mid table"""
    rng = np.random.default_rng(seed + 11)
    src = [s for s in mid_reads(k, seed) + big_reads(k, seed, canonical) if len(s) >= 2 * k]
    reads = []
    while len(reads) < 32:
        s = src[int(rng.integers(0, len(src)))]
        n = int(rng.integers(0, min(300, len(s)) + 1))
        a = int(rng.integers(0, len(s) - n + 1))
        r = s[a:a + n]
        if rng.integers(0, 2):
            r = gm.revcomp(r)
        what = int(rng.integers(0, 6))
        if n > k and what < 3:
            p = int(rng.integers(0, n))
            r = r[:p] + ("ACGT"[("ACGT".index(r[p]) + 1) % 4] if what == 0 else "N" if what == 1 else r[p].lower()) + r[p + 1:]
        reads.append(r)
    g = [s for s in big_reads(k, seed, canonical) if len(s) > chunk_inputs.CHUNK + 83][0]
    reads += ["", g[5:5 + chunk_inputs.CHUNK + 83]] + ti.repeat(k, seed)[1][:6]
    assert len(reads) % 2 == 0
    return reads


def batch_b(k, seed):
    """a second batch whose byte length is odd (the 16-byte padding rule): the reads that span the mid table's repeat on
    the ways the first batch leaves out, the bubble's two arms, twice round the cycle"""
    reads = ti.repeat(k, seed)[1][6:] + [bi.substitution(k, seed + 1)[2], bi.substitution(k, seed + 1)[1][2 * k:4 * k + 5]] + mi.circular(k, seed + 2, 20)[1]
    if len(reads) % 2:
        reads.append("ACGTN")
    if sum(map(len, reads)) % 2 == 0:
        reads[-1] += "A"
    return reads


def pack_key(kmer):
    v = 0
    for ch in kmer:
        v = v * 4 + "ACGT".index(ch)
    return v >> 64, v & M64


def arrays_of(table):
    """(key_hi, key_lo, count) of a {k-mer: count} in view order: keys packed MSB-first, ascending"""
    keys = sorted(table)
    packed = [pack_key(x) for x in keys]
    return (np.array([p[0] for p in packed], U64), np.array([p[1] for p in packed], U64), np.array([table[x] for x in keys], U64))


def _words(w):
    return np.array(w, U64)


def _bytes(s):
    return np.frombuffer(s.encode(), U8).copy()


def _kept(table, kept):
    hi, lo, cnt = arrays_of(kept)
    return [("key_hi", hi), ("key_lo", lo), ("count", cnt)]


class Menu:
    """Everything of one configuration (k, canonical): tables, batches, memoised expected values."""

    def __init__(self, k, canonical, seed=0):
        self.k, self.canonical, self.seed = k, canonical, 1000 + k + seed
        self.reads = {"few": few_reads(k, self.seed), "mid": mid_reads(k, self.seed), "big": big_reads(k, self.seed, canonical), "empty": []}
        self.batches = (batch_a(k, self.seed, canonical), batch_b(k, self.seed))
        self.packed = tuple(mi.pack(b) for b in self.batches)
        self._tables, self._arrays, self._graphs, self._memo, self._counts = {}, {}, {}, {}, {}

    # ---- tables ----
    def table(self, tid):
        if tid not in self._tables:
            if tid[0] == "kept":
                _, src, kind, rng, limits = tid
                self._tables[tid] = dict(self._cleaned(src, kind, rng, limits).kept)
            else:
                t = gm.count_table(self.reads[tid[0]], self.k, self.canonical)
                self._tables[tid] = {x: c * tid[1] for x, c in t.items()}
        return self._tables[tid]

    def arrays(self, tid):
        if tid not in self._arrays:
            self._arrays[tid] = arrays_of(self.table(tid))
        return self._arrays[tid]

    def graph(self, tid, rng):
        """(unitig model, links model) of a table and range"""
        if (tid, rng) not in self._graphs:
            t = self.table(tid)
            if t:
                g = (um.unitigs(t, self.canonical, *rng), lm.links(t, self.canonical, *rng))
            else:
                g = (um.Unitigs([], [], [], 0, self.k), lm.Links([0], [], 0, self.k))
            self._graphs[(tid, rng)] = g
        return self._graphs[(tid, rng)]

    def _cleaned(self, tid, kind, rng, limits):
        t, g = self.table(tid), self.graph(tid, rng)
        if kind == "clean":
            return cm.clean(t, self.canonical, *rng, *limits, graph=g)
        if kind == "simplify":
            return bm.simplify(t, self.canonical, *rng, *limits, graph=g)
        return pm.components(t, self.canonical, *rng, *limits, graph=g)

    def window_counts(self, tid, batch):
        if (tid, batch) not in self._counts:
            self._counts[(tid, batch)] = nm.all_counts(self.table(tid), self.canonical, self.batches[batch], self.k)
        return self._counts[(tid, batch)]

    def query_keys(self, tid):
        """every fifth key of the table, each also with its lowest bit flipped (mostly absent), and key 0"""
        hi, lo, _ = self.arrays(("mid", 1) if tid is None or tid[0] in ("empty", "kept") else (tid[0], 1))
        hi, lo = hi[::5], lo[::5]
        return np.concatenate([hi, hi, np.zeros(1, U64)]), np.concatenate([lo, lo ^ U64(1), np.zeros(1, U64)])

    # ---- expected values ----
    def expected(self, tid, family, args, partner=None):
        key = (tid, family, args, partner)
        if key not in self._memo:
            self._memo[key] = OrderedDict(getattr(self, "_x_" + family)(tid, *args) if partner is None else
                                          getattr(self, "_x_" + family)(tid, *args, partner=partner))
        return self._memo[key]

    def _x_export(self, tid):
        hi, lo, cnt = self.arrays(tid)
        return [("key_hi", hi), ("key_lo", lo), ("count", cnt)]

    def _x_partition(self, tid, n_parts):
        """part_begin and the table in (owner, key) order: the order inside a part is arbitrary, the test sorts each part"""
        kd = importlib.import_module("k-mer-count_amd.distributed")
        hi, lo, cnt = self.arrays(tid)
        own = kd.owner_np(hi, lo, n_parts) if len(lo) else np.zeros(0, np.int64)
        begin = np.zeros(n_parts + 1, U64)
        begin[1:] = np.cumsum(np.bincount(own, minlength=n_parts))
        order = np.argsort(own, kind="stable")
        return [("part_begin", begin), ("key_hi", hi[order]), ("key_lo", lo[order]), ("count", cnt[order])]

    def _ranged(self, tid, rng):
        hi, lo, cnt = self.arrays(tid)
        keep = (cnt >= U64(max(rng[0], 1))) & ((cnt <= U64(rng[1])) if rng[1] else np.ones(len(cnt), bool))
        return hi[keep], lo[keep], cnt[keep]

    def _x_histogram(self, tid, rng):
        c = [int(x) for x in self._ranged(tid, rng)[2]]
        hist = np.zeros(HIST_BINS, U64)
        for x in c:
            hist[min(x, HIST_BINS - 1)] += U64(1)
        return [("hist", hist), ("words", _words([max(c, default=0)]))]

    def _x_filter(self, tid, rng):
        hi, lo, cnt = self._ranged(tid, rng)
        return [("key_hi", hi), ("key_lo", lo), ("count", cnt), ("words", _words([len(lo), int(cnt.sum(dtype=U64)) if len(cnt) else 0]))]

    def _x_query(self, tid):
        t = {pack_key(x): c for x, c in self.table(tid).items()}
        hi, lo = self.query_keys(tid)
        return [("count", np.array([t.get((int(h), int(l)), 0) for h, l in zip(hi, lo)], U64))]

    def _x_profile(self, tid, batch, min_count):
        counts = self.window_counts(tid, batch)
        win, stats = [], []
        for read, c in zip(self.batches[batch], counts):
            win += [x or 0 for x in c] + [0] * (len(read) - len(c))
            v = [x for x in c if x is not None]
            full = [self.table(tid).get(gm.canon(read[j:j + self.k], self.canonical), 0) for j, x in enumerate(c) if x is not None]
            stats.append([len(v), sum(1 for x in full if x >= max(min_count, 1)), min(full, default=0), max(full, default=0), sum(full)])
        return [("window_count", np.array(win, U32)), ("read_stats", np.array(stats, U64).reshape(-1, 5))]

    def _x_compare(self, tid, variant, rng_a, rng_b, partner=None):
        a, b = self.arrays(tid), self.arrays(partner)
        lim = (max(rng_a[0], 1), rng_a[1], max(rng_b[0], 1), rng_b[1])
        words = ("words", _words(so.summary(a, b, *lim)))
        if variant[0] == "compare":
            return [words]
        (hi, lo, cnt), total = so.setop(a, b, variant[1], variant[2], *lim)
        return [("key_hi", hi), ("key_lo", lo), ("count", cnt), ("totals", _words([len(lo), total])), words]

    def _x_graph(self, tid, rng):
        _, adj, words = gm.graph(self.table(tid), self.canonical, *rng)
        return [("adj", np.array(adj, U16)), ("words", _words(words))]

    def _x_unitigs(self, tid, rng):
        u = self.graph(tid, rng)[0]
        return [("bases", _bytes(u.bases)), ("offsets", np.array(u.offsets, U64)), ("abund", np.array(u.abund, U64)),
                ("flags", np.array(u.flags, U8)), ("words", _words(u.summary))]

    def _x_links(self, tid, rng):
        u, lk = self.graph(tid, rng)
        words = lk.summary if len(u.seqs) else [0] * 8
        return [("link_offsets", np.array(lk.offsets, U64)), ("link_to", np.array(lk.to, U32)), ("words", _words(words))]

    def _map(self, tid, rng, batch):
        key = ("map", tid, rng, batch)
        if key not in self._memo:
            self._memo[key] = mm.ReadMap(self.batches[batch], self.k, self.canonical, self.graph(tid, rng)[0].seqs)
        return self._memo[key]

    def _x_map(self, tid, rng, batch):
        m = self._map(tid, rng, batch)
        return [("place", np.array(m.place, U64)), ("read_stats", np.array(m.stats, U32).reshape(-1, 4)), ("seg_offsets", np.array(m.seg_offsets, U64)),
                ("segs", np.array(m.segments, U32).reshape(-1, 4)), ("support", np.array(m.support, U64)), ("words", _words(m.summary))]

    def _x_transits(self, tid, rng, batches, min_reads):
        """batches: the batches the ledger says have been added, this call's last"""
        u, lk = self.graph(tid, rng)
        t = tm.Transits(lk, len(u.seqs), self.k)
        for b in batches:
            t.add(self._map(tid, rng, b).read_segments)
        t.judge(min_reads)
        return [("link_support", np.array(t.link_support, U64)), ("transit_offsets", np.array(t.transit_offsets, U64)),
                ("transit_count", np.array(t.transit_count, U64)), ("verdict", np.array(t.verdict, U8)), ("words", _words(t.summary))]

    def _x_correct(self, tid, rng, batch):
        c = crm.Corrected(self.batches[batch], self.k, self.canonical, gm.solid_set(self.table(tid), *rng))
        return [("corrected", _bytes("".join(c.corrected))), ("read_stats", np.array(c.stats, U32).reshape(-1, 4)),
                ("cand_offsets", np.array(c.cand_offsets, U64)), ("cands", np.array(c.cands, U32).reshape(-1, 4)), ("words", _words(c.summary))]

    def _x_trim(self, tid, rng, batch, rule):
        mode, flags, min_strong, min_permille, min_len = rule
        t = trm.Trimmed(self.batches[batch], self.k, self.canonical, gm.solid_set(self.table(tid), *rng), mode, flags, min_strong, min_permille, min_len)
        return self._emitted(t)

    def _emitted(self, t):
        return [("out_bases", _bytes("".join(t.out))), ("out_offsets", np.array(t.offsets, U64)), ("origin", np.array(t.origin, U64)),
                ("read_stats", np.array(t.stats, U32).reshape(-1, 4)), ("verdict", np.array(t.verdict, U8)), ("words", _words(t.summary))]

    def _x_normalize(self, tid, batch, rule):
        permille, target, min_depth, seed, flags = rule
        return self._emitted(nm.Normalized(self.batches[batch], self.window_counts(tid, batch), permille, target, min_depth, seed, flags))

    def _x_clean(self, tid, rng, limits):
        c = self._cleaned(tid, "clean", rng, limits)
        return _kept(self.table(tid), c.kept) + [("verdict", np.array(c.verdict, U8)), ("words", _words(c.summary))]

    def _x_simplify(self, tid, rng, limits):
        c = self._cleaned(tid, "simplify", rng, limits)
        return _kept(self.table(tid), c.kept) + [("verdict", np.array(c.verdict, U8)), ("words", _words(c.summary))]

    def _x_components(self, tid, rng, limits):
        c = self._cleaned(tid, "components", rng, limits)
        return [("comp_of", np.array(c.comp_of, U32)), ("comp_stats", np.array(c.stats, U64).reshape(-1, 4)), ("verdict", np.array(c.verdict, U8))] + \
            _kept(self.table(tid), c.kept) + [("words", _words(c.summary))]

    def _x_bubbles(self, tid, rng, limits):
        t = self.table(tid)
        if not t:
            return [("records", np.zeros((0, 8), U32)), ("words", _words([0] * 8))]
        c = bcm.calls(t, self.canonical, *rng, limits[0], graph=self.graph(tid, rng))
        return [("records", np.array(c.records, U32).reshape(-1, 8)), ("words", _words(c.summary))]

    def _x_into(self, tid, kind, rng, limits):
        """the summary words of the call; the partner then holds ("kept", tid, kind, rng, limits)"""
        return [("words", _words(self._cleaned(tid, kind, rng, limits).summary))]
