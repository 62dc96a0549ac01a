"""The model of the two-table calls (kmc_compare / kmc_setop_device / kmc_export_setop): a plain numpy restatement of
the semantics table of include/kmc.h on (key_hi, key_lo, count) arrays.  It shares no code with the library.

A table is a tuple (key_hi, key_lo, count) of uint64 arrays with unique keys (any order).  All arithmetic is uint64
with wrap-around, which is what "plain 64-bit addition" in the header means."""
import numpy as np

INTERSECT, UNION, SUBTRACT = 0, 1, 2
LEFT, RIGHT, MIN, MAX, SUM, DIFF = 0, 1, 2, 3, 4, 5
OPS = (INTERSECT, UNION, SUBTRACT)
MODES = (LEFT, RIGHT, MIN, MAX, SUM, DIFF)
OP_NAMES = {"intersect": INTERSECT, "union": UNION, "subtract": SUBTRACT}
MODE_NAMES = {"left": LEFT, "right": RIGHT, "min": MIN, "max": MAX, "sum": SUM, "diff": DIFF}
WORD_NAMES = ("n_a", "n_b", "n_both", "sum_a", "sum_b", "shared_sum_a", "shared_sum_b", "sum_min")

U = np.uint64


def table(key_hi, key_lo, count):
    return (np.asarray(key_hi, U).ravel(), np.asarray(key_lo, U).ravel(), np.asarray(count, U).ravel())


def of(t):
    """(key_hi, key_lo, count) of anything with these three attributes (the library's Table, the oracle's)."""
    return table(t.key_hi, t.key_lo, t.count)


def _ranged(count, lo, hi):
    c = np.asarray(count, U)
    ok = c >= U(lo)
    if hi:
        ok &= c <= U(hi)
    return np.where(ok, c, U(0))


def join(a, b, min_a=1, max_a=0, min_b=1, max_b=0):
    """Every key of either table, ascending, with ca / cb (0 = absent or outside its range); keys with ca == cb == 0 dropped."""
    hi = np.concatenate([a[0], b[0]])
    lo = np.concatenate([a[1], b[1]])
    c = np.concatenate([_ranged(a[2], min_a, max_a), _ranged(b[2], min_b, max_b)])
    side = np.concatenate([np.zeros(a[1].shape[0], np.int8), np.ones(b[1].shape[0], np.int8)])
    order = np.lexsort((lo, hi))
    hi, lo, c, side = hi[order], lo[order], c[order], side[order]
    n = hi.shape[0]
    first = np.ones(n, bool)
    if n > 1:
        first[1:] = (hi[1:] != hi[:-1]) | (lo[1:] != lo[:-1])
    gid = np.cumsum(first) - 1
    ng = int(gid[-1]) + 1 if n else 0
    ca, cb = np.zeros(ng, U), np.zeros(ng, U)
    ca[gid[side == 0]] = c[side == 0]
    cb[gid[side == 1]] = c[side == 1]
    khi, klo = hi[first], lo[first]
    live = (ca != 0) | (cb != 0)
    return khi[live], klo[live], ca[live], cb[live]


def summary(a, b, min_a=1, max_a=0, min_b=1, max_b=0):
    """The eight words, as Python ints (sums modulo 2^64)."""
    _, _, ca, cb = join(a, b, min_a, max_a, min_b, max_b)
    both = (ca != 0) & (cb != 0)
    s = lambda x: int(x.sum(dtype=U)) if x.shape[0] else 0
    return [int((ca != 0).sum()), int((cb != 0).sum()), int(both.sum()), s(ca), s(cb), s(ca[both]), s(cb[both]),
            s(np.minimum(ca, cb)[both])]


def setop(a, b, op, mode, min_a=1, max_a=0, min_b=1, max_b=0):
    """(key_hi, key_lo, count) of the result, ascending, and total_out (sum of the result counts modulo 2^64)."""
    khi, klo, ca, cb = join(a, b, min_a, max_a, min_b, max_b)
    ina, inb = ca != 0, cb != 0
    sel = {INTERSECT: ina & inb, UNION: ina | inb, SUBTRACT: ina & ~inb}[op]
    r = {LEFT: ca, RIGHT: cb, MIN: np.minimum(ca, cb), MAX: np.maximum(ca, cb), SUM: ca + cb,
         DIFF: np.where(ca > cb, ca - cb, U(0))}[mode]
    keep = sel & (r != 0)
    out = (khi[keep], klo[keep], r[keep])
    return out, (int(out[2].sum(dtype=U)) if out[2].shape[0] else 0)


def similarities(w):
    """union and the derived similarities of the eight words; a zero denominator gives 0.0."""
    div = lambda x, y: x / y if y else 0.0
    union = w[0] + w[1] - w[2]
    return {"union": union, "jaccard": div(w[2], union), "containment_a": div(w[2], w[0]), "containment_b": div(w[2], w[1]),
            "weighted_jaccard": div(w[7], w[3] + w[4] - w[7]), "bray_curtis": div(2 * w[7], w[3] + w[4])}


def compare_text(w):
    """What the CLI's --compare prints."""
    s = similarities(w)
    lines = ["%s\t%d" % (n, v) for n, v in zip(WORD_NAMES, w)] + ["union\t%d" % s["union"]]
    lines += ["%s\t%.6f" % (n, s[n]) for n in ("jaccard", "containment_a", "containment_b", "weighted_jaccard", "bray_curtis")]
    return ("\n".join(lines) + "\n").encode()


def table_text(t, klen):
    """KMER<TAB>COUNT lines of a result (keys packed MSB-first, A=0 C=1 G=2 T=3)."""
    out = []
    for h, l, c in zip(t[0].tolist(), t[1].tolist(), t[2].tolist()):
        v = (h << 64) | l
        out.append("".join("ACGT"[(v >> (2 * (klen - 1 - i))) & 3] for i in range(klen)) + "\t%d\n" % c)
    return "".join(out).encode()
