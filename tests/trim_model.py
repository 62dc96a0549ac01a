"""kmc_trim restated on Python strings (include/kmc.h): windows strong or not against the solid part of a table, the strong
runs of a read, its span by mode, PASS, pairs, INVERT, the emitted batch and the summary.  On correct_model's windows and
graph_model's solid_set; nothing here shares code with the kernels.  CPU only."""
import correct_model as cm
import graph_model as gm

NONE, ENDS, LONGEST = 0, 1, 2
INVERT, PAIR_BOTH, PAIR_EITHER = 1, 2, 4
PASS, EMITTED = 1, 2
MODE_NAMES = {"none": NONE, "ends": ENDS, "longest": LONGEST}


def strong_runs(strong):
    """[(start, length)] of the maximal runs of True"""
    runs, j, n = [], 0, len(strong)
    while j < n:
        if not strong[j]:
            j += 1
            continue
        a = j
        while j < n and strong[j]:
            j += 1
        runs.append((a, j - a))
    return runs


def read_words(read, k, canonical, solid):
    """(V, S, F, E, B, N, runs) of a read; F, E, B, N are 0 without a strong window"""
    w = cm.windows(read, k, canonical, solid)      # None: not valid, True: weak, False: strong
    strong = [x is False for x in w]
    V, S = sum(x is not None for x in w), sum(strong)
    runs = strong_runs(strong)
    if not S:
        return V, 0, 0, 0, 0, 0, runs
    F, E = strong.index(True), len(strong) - 1 - strong[::-1].index(True)
    N = max(n for _, n in runs)
    B = min(a for a, n in runs if n == N)
    return V, S, F, E, B, N, runs


def span_of(words, L, k, mode):
    V, S, F, E, B, N = words[:6]
    if mode == NONE:
        return 0, L
    if not S:
        return 0, 0
    return (F, E - F + k) if mode == ENDS else (B, N + k - 1)


def passes(words, length, mode, min_strong, min_permille, min_len):
    V, S = words[0], words[1]
    return S >= min_strong and S * 1000 >= min_permille * V and length >= min_len and (mode == NONE or S > 0)


class Trimmed:
    """out (strings), origin, stats [n_reads][4], verdict [n_reads], summary [8], offsets [n_out + 1]"""

    def __init__(self, reads, k, canonical, solid, mode=LONGEST, flags=0, min_strong=0, min_permille=0, min_len=0, words=None):
        assert mode in (NONE, ENDS, LONGEST) and not flags & ~7 and min_permille <= 1000
        assert not (flags & PAIR_BOTH and flags & PAIR_EITHER) and not (flags & INVERT and mode != NONE)
        assert not (flags & (PAIR_BOTH | PAIR_EITHER) and len(reads) & 1)
        self.reads, self.k, self.mode = list(reads), k, mode
        self.words = words or [read_words(r, k, canonical, solid) for r in self.reads]      # (words: those of an earlier call, same reads and solid set)
        self.stats, own = [], []
        for r, w in zip(self.reads, self.words):
            start, length = span_of(w, len(r), k, mode)
            self.stats.append([w[0], w[1], start, length])
            own.append(passes(w, length, mode, min_strong, min_permille, min_len))
        verdicts = list(own)
        if flags & (PAIR_BOTH | PAIR_EITHER):
            for i in range(0, len(own), 2):
                v = (own[i] and own[i + 1]) if flags & PAIR_BOTH else (own[i] or own[i + 1])
                verdicts[i] = verdicts[i + 1] = v
        emitted = [v != bool(flags & INVERT) for v in verdicts]
        self.verdict = [(PASS if p else 0) | (EMITTED if e else 0) for p, e in zip(own, emitted)]
        self.origin = [i for i, e in enumerate(emitted) if e]
        self.out = [self.reads[i][self.stats[i][2]:self.stats[i][2] + self.stats[i][3]] for i in self.origin]
        self.offsets = [0]
        for s in self.out:
            self.offsets.append(self.offsets[-1] + len(s))
        self.summary = [len(self.reads), sum(s[0] for s in self.stats), sum(s[1] for s in self.stats), sum(own), len(self.out), self.offsets[-1],
                        sum(1 for i in self.origin if self.stats[i][3] < len(self.reads[i])), sum(len(self.reads[i]) for i in self.origin)]

    def text(self):
        """what ``k-mer-count --trim`` prints"""
        return "".join(">%d %d %d %d %d\n%s\n" % (i, *self.stats[i], s) for i, s in zip(self.origin, self.out))


def trim_reads(table, canonical, reads, min_count=1, max_count=0, k=None, **rule):
    """table: {k-mer string: count}; k is needed for an empty table; rule: mode, flags, min_strong, min_permille, min_len"""
    if k is None:
        k = len(next(iter(table)))
    return Trimmed(reads, k, canonical, gm.solid_set(table, min_count, max_count), **rule)
