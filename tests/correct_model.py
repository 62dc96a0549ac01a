"""kmc_correct restated on Python strings (include/kmc.h): windows weak or strong against the solid part of a table, weak
runs and their borders, candidates, the accepted replacements, the corrected reads.  On graph_model's canon / solid_set;
nothing here shares code with the kernels.  CPU only."""
import graph_model as gm

BASES = "ACGT"
INTERIOR, HEAD, TAIL = 0, 1, 2
START, SOLID, INVALID, END = "START", "SOLID", "INVALID", "END"
KIND_NAMES = ("INTERIOR", "HEAD", "TAIL")


def windows(read, k, canonical, solid):
    """per window of the read: None (not valid), True (weak) or False (strong)"""
    out = []
    for j in range(len(read) - k + 1):
        f = read[j:j + k]
        out.append(None if f.strip(BASES) else gm.canon(f, canonical) not in solid)
    return out


def weak_runs(weak):
    """[(a, b, left border, right border)] of the maximal runs of weak windows"""
    runs, j, n = [], 0, len(weak)
    while j < n:
        if weak[j] is not True:
            j += 1
            continue
        a = j
        while j + 1 < n and weak[j + 1] is True:
            j += 1
        b = j
        left = START if a == 0 else SOLID if weak[a - 1] is False else INVALID
        right = END if b == n - 1 else SOLID if weak[b + 1] is False else INVALID
        runs.append((a, b, left, right))
        j += 1
    return runs


def candidate_of(run, k):
    """(kind, p) of a weak run, or None"""
    a, b, left, right = run
    n = b - a + 1
    if left == SOLID and right == SOLID and n == k:
        return INTERIOR, b
    if left == START and right == SOLID and n <= k:
        return HEAD, b
    if left == SOLID and right == END and n <= k:
        return TAIL, a + k - 1
    return None


def accepted_mask(read, k, canonical, solid, a, b, p):
    mask = 0
    for code, c in enumerate(BASES):
        if c == read[p]:
            continue
        s = read[:p] + c + read[p + 1:]
        if all(gm.canon(s[j:j + k], canonical) in solid for j in range(a, b + 1)):
            mask |= 1 << code
    return mask


def correct_read(read, k, canonical, solid):
    """(corrected read, [valid, weak, candidates, corrected], records [p, word, a, n], weak runs, ambiguous, windows fixed):
    every candidate is tested against the read as it came"""
    weak = windows(read, k, canonical, solid)
    runs = weak_runs(weak)
    out, recs, n_amb, fixed_windows, n_fixed = list(read), [], 0, 0, 0
    ps = []
    for run in runs:
        c = candidate_of(run, k)
        if c is None:
            continue
        kind, p = c
        a, b = run[0], run[1]
        # INDEPENDENCE (kmc.h): the windows a..b are exactly those of the read that contain p ...
        assert [j for j in range(len(weak)) if j <= p < j + k] == list(range(a, b + 1)), (read, run, p)
        ps.append((a, b, p))
        mask = accepted_mask(read, k, canonical, solid, a, b, p)
        new = read[p]
        if bin(mask).count("1") == 1:
            new = BASES[mask.bit_length() - 1]
            out[p] = new
            n_fixed += 1
            fixed_windows += b - a + 1
        elif mask:
            n_amb += 1
        recs.append([p, ord(read[p]) | ord(new) << 8 | kind << 16 | mask << 24, a, b - a + 1])
    # ... and two suspect positions are more than k - 1 apart, so nobody's windows hold another's p
    for i, (a, b, p) in enumerate(ps):
        for j, (_, _, q) in enumerate(ps):
            assert i == j or (abs(p - q) > k - 1 and not a <= q < b + k), (read, ps)
    nv = sum(w is not None for w in weak)
    nw = sum(w is True for w in weak)
    return "".join(out), [nv, nw, len(recs), n_fixed], recs, len(runs), n_amb, fixed_windows


class Corrected:
    """corrected (strings), stats [n_reads][4], cand_offsets [n_reads + 1], cands [n_cands][4], summary [8]"""

    def __init__(self, reads, k, canonical, solid):
        self.reads, self.k = list(reads), k
        self.corrected, self.stats, self.cand_offsets, self.cands = [], [], [0], []
        w = [len(self.reads), 0, 0, 0, 0, 0, 0, 0]
        fixed_windows = 0
        for r in self.reads:
            s, st, recs, n_runs, n_amb, fw = correct_read(r, k, canonical, solid)
            self.corrected.append(s)
            self.stats.append(st)
            self.cands += recs
            self.cand_offsets.append(len(self.cands))
            w[1] += st[0]; w[2] += st[1]; w[3] += n_runs; w[4] += st[2]; w[5] += st[3]; w[6] += n_amb
            fixed_windows += fw
        w[7] = w[2] - fixed_windows
        self.summary = w

    def fixes(self):
        """(read, pos, old, new, kind) of every corrected candidate"""
        out = []
        for r in range(len(self.reads)):
            for p, word, _, _ in self.cands[self.cand_offsets[r]:self.cand_offsets[r + 1]]:
                if (word & 255) != (word >> 8 & 255):
                    out.append((r, p, chr(word & 255), chr(word >> 8 & 255), word >> 16 & 255))
        return out

    def text(self):
        """what ``k-mer-count --correct`` prints"""
        return "".join(">%d %d %d %d %d\n%s\n" % (i, s[0], s[1], s[2], s[3], c) for i, (s, c) in enumerate(zip(self.stats, self.corrected)))


def correct_reads(table, canonical, reads, min_count=1, max_count=0, k=None):
    """table: {k-mer string: count}; k is needed for an empty table"""
    if k is None:
        k = len(next(iter(table)))
    return Corrected(reads, k, canonical, gm.solid_set(table, min_count, max_count))


def sequentially(table, canonical, reads, min_count=1, max_count=0, k=None, reverse=False):
    """The restatement of INDEPENDENCE: a read's candidates are found once, then each is tested and applied in turn on the
    read as corrected so far (from the last to the first with reverse)"""
    if k is None:
        k = len(next(iter(table)))
    solid = gm.solid_set(table, min_count, max_count)
    out = []
    for read in reads:
        cands = [(run, candidate_of(run, k)) for run in weak_runs(windows(read, k, canonical, solid))]
        cands = [(run[0], run[1], c[1]) for run, c in cands if c]
        s = read
        for a, b, p in (reversed(cands) if reverse else cands):
            mask = accepted_mask(s, k, canonical, solid, a, b, p)
            if bin(mask).count("1") == 1:
                s = s[:p] + BASES[mask.bit_length() - 1] + s[p + 1:]
        out.append(s)
    return out
