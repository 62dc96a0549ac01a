"""Walks one generated sequence (view_sequences.py) on a real ctx and checks every step (GPU; used by
tests/test_view_sequences_gpu.py in-process and, for the trace cases, in a child process).

After every step: the return code is the ledger's; the result -- arrays and summary words -- equals the expected value of
(the view's table, the arguments) byte for byte (view_expected.py); every device result handed out earlier that the
ledger still calls valid is read again through the pointers saved at the time and equals the host copy taken right after
its call (a pointer the ledger ends is dropped and never read); kmc_export_device still returns the view's pointers and
the view's bytes are unchanged.  A mismatch raises Mismatch, whose message names the configuration, the seed, the step,
the last ten steps and the first differing array: the case can be run again from it."""
import ctypes as C
import sys
from collections import OrderedDict

import numpy as np

import map_inputs as mi
import view_expected as vx
import view_ledger as vl
import view_sequences as vs
from test_unitig_gpu import _dev_bytes     # (n bytes at a device address)

U64, U32, U16, U8 = np.uint64, np.uint32, np.uint16, np.uint8


class Mismatch(AssertionError):
    pass


class Runner:
    def __init__(self, kmc, menu, k, canonical, seed, steps, mark=None):
        import torch
        self.kmc, self.m, self.k, self.canonical, self.seed, self.steps = kmc, menu, k, canonical, seed, steps
        self.L = kmc.lib()
        self.two = k > 32
        self.mark = mark or (lambda text: None)      # the trace cases: a line on stderr in front of what a step prints
        self.kc = kmc.KmerCounter(k=k, canonical=canonical)
        self.pc = kmc.KmerCounter(k=k, canonical=canonical)
        self.dev = torch.device("cuda", 0)
        self.batches = []                            # per batch: host bases, offsets, device tensors (kept alive)
        for bases, offs in menu.packed:
            db = torch.zeros(len(bases) + 64, dtype=torch.uint8, device=self.dev)
            db[:len(bases)] = torch.from_numpy(bases.copy())
            do = torch.from_numpy(offs.view(np.int64).copy()).to(self.dev)
            self.batches.append((bases, offs, db, do))
        torch.cuda.synchronize(self.dev)
        self._count(self.pc, "few")
        self.held = vs.Held()
        self.trim_calls = 0
        self.view_ptrs = self.view_copy = None
        self.n_results = self.n_reread = 0           # results compared, held results read again

    def close(self):
        self.kc.close()
        self.pc.close()

    # ---- helpers ----
    def _count(self, ctx, table, reset=True, finalize="sync"):
        if reset:
            ctx.reset()
        ctx.add_batch(*mi.pack(self.m.reads[table]))
        if finalize == "sync":
            ctx.finalize()
        else:
            ctx.finalize_async()

    def _fail(self, step, what, got=None, want=None):
        first = max(0, step.idx - 9)
        lines = ["view sequence k=%d canonical=%s seed=%d step %d: %s" % (self.k, self.canonical, self.seed, step.idx, what)]
        if got is not None:
            g, w = np.asarray(got).ravel(), np.asarray(want).ravel()
            n = min(len(g), len(w))
            bad = np.flatnonzero(g[:n] != w[:n])[:5]
            lines.append("  sizes %d / %d, first differing entries %s: got %s, expected %s" % (len(g), len(w), bad.tolist(), g[bad].tolist(), w[bad].tolist()))
        lines += ["  " + s.text() for s in self.steps[first:step.idx + 1]]
        raise Mismatch("\n".join(lines))

    def _triple(self, ptrs, n):
        """[(name, ptr, bytes, dtype)] of a device (key_hi, key_lo, count) result; one-word keys have no high words"""
        return [("key_hi", ptrs[0] if self.two else 0, 8 * n, U64), ("key_lo", ptrs[1], 8 * n, U64), ("count", ptrs[2], 8 * n, U64)]

    def _read(self, spec):
        """{name: array} of [(name, ptr, bytes, dtype)]; a NULL pointer stands for zeros (key_hi of one-word keys)"""
        out = OrderedDict()
        for name, ptr, nbytes, dtype in spec:
            out[name] = _dev_bytes(ptr, nbytes).view(dtype) if ptr else np.zeros(nbytes // np.dtype(dtype).itemsize, dtype)
        return out

    def _table(self, t):
        return OrderedDict([("key_hi", t.key_hi), ("key_lo", t.key_lo), ("count", t.count)])

    # ---- producers ----
    def produce(self, s):
        kc, pc = self.kc, self.pc
        self.mark("produce")
        if s.name == "fresh":
            self._count(kc, s.table)
        elif s.name == "async":
            self._count(kc, s.table, finalize="async")
        elif s.name == "double":
            if s.args[0]:
                self._count(kc, s.table)
            self._count(kc, s.table, reset=False)
        elif s.name == "refinalize":
            kc.finalize()
        elif s.name == "empty":
            kc.reset()
            kc.finalize()
        elif s.name == "none":
            kc.reset()
        elif s.name == "merge":
            self._count(pc, s.table)
            hi, lo, cnt, n = pc.export_device()
            kc.reset()
            kc.merge_pairs_device(hi, lo, cnt, n)
            kc.finalize()
        if s.outcome.ended:                  # (a finalize with nothing added keeps the view: the same pointers, the same bytes)
            self.view_ptrs = self.view_copy = None

    # ---- one family call on a ctx: (result, device spec or None) ----
    def run(self, ctx, family, form, args, want, partner=None, accumulate=False):
        kmc, L, two = self.kmc, self.L, self.two
        words = lambda summary: np.array(summary.words(), U64)
        n_of = lambda name: int(want[name].shape[0])
        if family == "export":
            ptrs = ctx.export_device()
            if form == "device":
                spec = self._triple(ptrs, ptrs[3])
                return self._read(spec), {"view": spec}
            n = ptrs[3]
            hi, lo, cnt = np.zeros(n, U64), np.zeros(n, U64), np.zeros(n, U64)
            ctx._chk(L.kmc_export(ctx._h, hi.ctypes.data, lo.ctypes.data, cnt.ctypes.data, n))
            return OrderedDict([("key_hi", hi), ("key_lo", lo), ("count", cnt)]), None
        if family == "partition":
            begin, *ptrs = ctx.partition_device(args[0])
            spec = self._triple(ptrs, begin[-1])
            got = self._read(spec)
            part = np.repeat(np.arange(args[0]), np.diff(np.array(begin, np.int64)))
            order = np.lexsort((got["key_lo"], got["key_hi"], part))           # (the order inside a part is arbitrary)
            out = OrderedDict([("part_begin", np.array(begin, U64))] + [(n, a[order]) for n, a in got.items()])
            return out, {"partition": spec}
        if family == "histogram":
            h, mx = ctx.histogram(vx.HIST_BINS, *args[0], return_max=True)
            return OrderedDict([("hist", h), ("words", np.array([mx], U64))]), None
        if family == "filter":
            if form == "host":
                return self._table(ctx.export_filtered(*args[0])), None
            *ptrs, n, total = ctx.filter_device(*args[0])
            spec = self._triple(ptrs, n)
            got = self._read(spec)
            got["words"] = np.array([n, total], U64)
            return got, {"filter": spec}
        if family == "query":
            hi, lo = self.m.query_keys(self.cur_table)
            if form == "host":
                return OrderedDict([("count", ctx.query(lo, hi if two else None))]), None
            import torch
            t = [torch.from_numpy(a.view(np.int64).copy()).to(self.dev) for a in (hi, lo)] + [torch.zeros(len(lo), dtype=torch.int64, device=self.dev)]
            torch.cuda.synchronize(self.dev)
            ctx.query_device(t[0].data_ptr() if two else 0, t[1].data_ptr(), len(lo), t[2].data_ptr())
            ctx.sync()
            return OrderedDict([("count", t[2].cpu().numpy().view(U64))]), None
        if family == "profile":
            bases, offs, db, do = self.batches[args[0]]
            if form == "host":
                win, rs = ctx.profile(bases, offs, args[1])
            else:
                win, rs = ctx.profile_tensors(db[:len(bases)], do, args[1])
                ctx.sync()
                win, rs = win.cpu().numpy().view(U32), rs.cpu().numpy().view(U64)
            return OrderedDict([("window_count", win), ("read_stats", rs)]), None
        if family == "compare":
            variant, ra, rb = args
            lim = (ra[0], ra[1], rb[0], rb[1])
            if variant[0] == "compare":
                return OrderedDict([("words", np.array(ctx.compare(partner, *lim).words(), U64))]), None
            if form == "host":
                return self._table(ctx.setop(partner, variant[1], variant[2], *lim)), None
            *ptrs, n, total, summary = ctx.setop_device(partner, variant[1], variant[2], *lim, return_summary=True)
            spec = self._triple(ptrs, n)
            got = self._read(spec)
            got["totals"], got["words"] = np.array([n, total], U64), np.array(summary.words(), U64)
            return got, {"setop": spec}
        if family == "graph":
            if form == "host":
                adj, summary = ctx.graph(*args[0])
                return OrderedDict([("adj", adj), ("words", words(summary))]), None
            ptr, n, summary = ctx.graph_device(*args[0])
            spec = [("adj", ptr, 2 * n, U16)]
            got = self._read(spec)
            got["words"] = words(summary)
            return got, {"adj": spec}
        if family == "unitigs":
            if form == "host":
                u = ctx.unitigs(*args[0])
                return OrderedDict([("bases", u.bases), ("offsets", u.offsets), ("abund", u.abund), ("flags", u.flags), ("words", words(u.summary))]), None
            db, do, da, df, nu, nb, summary = ctx.unitigs_device(*args[0])
            spec = [("bases", db, nb, U8), ("offsets", do, 8 * (nu + 1), U64), ("abund", da, 8 * nu, U64), ("flags", df, nu, U8)]
            got = self._read(spec)
            got["words"] = words(summary)
            return got, {"unitig_arrays": spec}
        if family == "links":
            if form == "host":
                lk = ctx.unitig_links(*args[0])
                return OrderedDict([("link_offsets", lk.offsets), ("link_to", lk.to), ("words", words(lk.summary))]), None
            do, dt, nu, nl, summary = ctx.unitig_links_device(*args[0])
            spec = [("link_offsets", do, 8 * (2 * nu + 1), U64), ("link_to", dt, 4 * nl, U32)]
            got = self._read(spec)
            got["words"] = words(summary)
            return got, {"link_arrays": spec}
        if family == "map":
            rng, b = args
            bases, offs, db, do = self.batches[b]
            nr, nb = len(offs) - 1, len(bases)
            if form == "host":
                from test_map_gpu import _raw
                (place, stats, so, segs, sup), w = _raw(kmc, ctx, *rng, bases, offs, n_of("segs"), n_of("support"))
                return OrderedDict([("place", place), ("read_stats", stats), ("seg_offsets", so), ("segs", segs), ("support", sup),
                                    ("words", np.array(w, U64))]), None
            dp, ds, dso, dg, du, ns, nu, summary = ctx.map_reads_device(db.data_ptr(), do.data_ptr(), nr, nb, *rng)
            spec = [("place", dp, 8 * nb, U64), ("read_stats", ds, 16 * nr, U32), ("seg_offsets", dso, 8 * (nr + 1), U64), ("segs", dg, 16 * ns, U32),
                    ("support", du, 8 * nu, U64)]
            got = self._read(spec)
            got["words"] = words(summary)
            return got, {"map_arrays": spec}
        if family == "transits":
            rng, _, min_reads = args
            b = self.cur_batch
            bases, offs, db, do = self.batches[b]
            if form == "host":
                from test_transits_gpu import _raw
                sizes = (n_of("verdict"), n_of("link_support"), n_of("transit_count"))
                (sup, to, cnt, vd), w = _raw(kmc, ctx, *rng, bases, offs, sizes, min_reads, kmc.TRANSIT_ACCUMULATE if accumulate else 0)
                return OrderedDict([("link_support", sup), ("transit_offsets", to), ("transit_count", cnt), ("verdict", vd), ("words", np.array(w, U64))]), None
            ds, dt, dc, dv, nu, nl, nsl, summary = ctx.transits_device(db.data_ptr(), do.data_ptr(), len(offs) - 1, len(bases), *rng, min_reads, accumulate)
            spec = [("link_support", ds, 8 * nl, U64), ("transit_offsets", dt, 8 * (nu + 1), U64), ("transit_count", dc, 8 * nsl, U64), ("verdict", dv, nu, U8)]
            got = self._read(spec)
            got["words"] = words(summary)
            return got, {"transits": spec}
        if family == "correct":
            rng, b = args
            bases, offs, db, do = self.batches[b]
            nr, nb = len(offs) - 1, len(bases)
            if form == "host":
                from test_correct_gpu import _raw
                (out, stats, co, cands), w = _raw(kmc, ctx, *rng, bases, offs, n_of("cands"))
                return OrderedDict([("corrected", out), ("read_stats", stats), ("cand_offsets", co), ("cands", cands), ("words", np.array(w, U64))]), None
            dbo, ds, dco, dc, nc, summary = ctx.correct_reads_device(db.data_ptr(), do.data_ptr(), nr, nb, *rng)
            spec = [("corrected", dbo, nb, U8), ("read_stats", ds, 16 * nr, U32), ("cand_offsets", dco, 8 * (nr + 1), U64), ("cands", dc, 16 * nc, U32)]
            got = self._read(spec)
            got["words"] = words(summary)
            return got, {"correct_arrays": spec}
        if family in ("trim", "normalize"):
            if family == "trim":
                rng, b, (mode, flags, ms, mp, ml) = args
                host = lambda bases, offs: ctx.trim_reads(bases, offs, *rng, mode, flags, ms, mp, ml)
                device = lambda db, do, nr, nb: ctx.trim_reads_device(db, do, nr, nb, *rng, mode, flags, ms, mp, ml)
            else:
                b, (permille, target, min_depth, seed, flags) = args
                host = lambda bases, offs: ctx.normalize_reads(bases, offs, target, permille, min_depth, seed, flags)
                device = lambda db, do, nr, nb: ctx.normalize_reads_device(db, do, nr, nb, target, permille, min_depth, seed, flags)
            bases, offs, db, do = self.batches[b]
            nr, nb = len(offs) - 1, len(bases)
            if form == "host":
                t = host(bases, offs)
                return OrderedDict([("out_bases", t.bases), ("out_offsets", t.offsets), ("origin", t.origin), ("read_stats", t.stats), ("verdict", t.verdict),
                                    ("words", words(t.summary))]), None
            dob, doo, dor, ds, dv, no, nob, summary = device(db.data_ptr(), do.data_ptr(), nr, nb)
            two_bufs = [("out_bases", dob, nob, U8), ("out_offsets", doo, 8 * (no + 1), U64)]
            rest = [("origin", dor, 8 * no, U64), ("read_stats", ds, 16 * nr, U32), ("verdict", dv, nr, U8)]
            got = self._read(two_bufs + rest)
            got["words"] = words(summary)
            return got, ({"trim_double": two_bufs, "trim_arrays": rest} if family == "trim" else {"normalize_arrays": two_bufs + rest})
        if family in ("clean", "simplify"):
            rng, lim = args
            host, device = (ctx.clean_unitigs, ctx.clean_unitigs_device) if family == "clean" else (ctx.simplify_unitigs, ctx.simplify_unitigs_device)
            if form == "host":
                c = host(*rng, *lim)
                got = self._table(c.table)
                got["verdict"], got["words"] = c.verdict, words(c.summary)
                return got, None
            *ptrs, dv, nk, nu, summary = device(*rng, *lim)
            spec = self._triple(ptrs, nk) + [("verdict", dv, nu, U8)]
            got = self._read(spec)
            got["words"] = words(summary)
            return got, {"clean": spec}
        if family == "components":
            rng, lim = args
            if form == "host":
                c = ctx.components(*rng, *lim)
                got = OrderedDict([("comp_of", c.comp_of), ("comp_stats", c.stats), ("verdict", c.verdict)])
                got.update(self._table(c.table))
                got["words"] = words(c.summary)
                return got, None
            dc, dst, dv, *ptrs, nc, nu, nk, summary = ctx.components_device(*rng, *lim)
            spec = [("comp_of", dc, 4 * nu, U32), ("comp_stats", dst, 32 * nc, U64), ("verdict", dv, nu, U8)] + self._triple(ptrs, nk)
            got = self._read(spec)
            got["words"] = words(summary)
            return got, {"components": spec}
        if family == "bubbles":
            rng, lim = args
            if form == "host":
                nr, nu = C.c_uint64(), C.c_uint64()
                w = (C.c_uint64 * kmc.BUBBLE_WORDS)()
                ctx._chk(L.kmc_unitig_bubbles(ctx._h, *rng, lim[0], None, 0, C.byref(nr), C.byref(nu), w))
                rec = np.zeros((nr.value, 8), U32)
                ctx._chk(L.kmc_unitig_bubbles(ctx._h, *rng, lim[0], rec.ctypes.data if nr.value else None, nr.value, C.byref(nr), C.byref(nu), w))
                return OrderedDict([("records", rec), ("words", np.array(list(w), U64))]), None
            dr, nr, nu, summary = ctx.bubbles_device(*rng, lim[0])
            spec = [("records", dr, 32 * nr, U32)]
            got = self._read(spec)
            got["words"] = words(summary)
            return got, {"bubbles": spec}
        if family == "into":
            kind, rng, lim = args
            call = {"clean": ctx.clean_into, "simplify": ctx.simplify_into, "components": ctx.components_into}[kind]
            return OrderedDict([("words", words(call(partner, *rng, *lim)))]), None
        raise KeyError(family)

    def compare(self, step, got, want, what):
        if not got:
            self._fail(step, what + ": no result")
        for name, g in got.items():
            w = want[name]
            g = np.asarray(g)
            if g.dtype != w.dtype or g.size != w.size or g.tobytes() != w.tobytes():
                self._fail(step, "%s: array %r differs (%s%s / %s%s)" % (what, name, g.dtype, g.shape, w.dtype, w.shape), g, w)

    # ---- one step ----
    def step(self, s):
        if s.kind == "produce":
            self.produce(s)
            self.held.apply(s, self.trim_calls)
            return
        kmc = self.kmc
        self.cur_table = s.view
        self.cur_batch = s.ledger_args.get("batch")
        want = self.m.expected(s.view, s.name, s.args, s.partner if s.name == "compare" else None) if s.outcome.rc == 0 else None
        if s.name == "into" and s.outcome.rc == 0:
            self.pc.reset()
        self.mark("step %d" % s.idx)
        try:
            got, spec = self.run(self.kc, s.name, s.form, s.args, want or self._sizes_of_nothing(s), self.pc, s.accumulate)
            rc = 0
        except kmc.KmcError as e:
            got, spec, rc = None, None, e.status
        if rc != s.outcome.rc:
            self._fail(s, "return code %d, the ledger says %d" % (rc, s.outcome.rc))
        if rc == 0:
            self.compare(s, got, want, "result")
            self.n_results += 1
            if s.name == "trim":
                self.trim_calls += len(vl.EXPANSION[("trim", s.form)])
            if s.name == "into":
                self.mark("partner")
                self.pc.finalize()
                kept = ("kept", s.view) + s.args
                self.cur_table = kept
                self.compare(s, self.run(self.pc, "export", "host", (), None)[0], self.m.expected(kept, "export", ()), "the partner's table behind the *_into call")
                f, fform, fargs = s.follow
                self.cur_batch = fargs[1][0] if f == "transits" else None
                fwant = self.m.expected(kept, f, fargs)
                self.compare(s, self.run(self.pc, f, fform, fargs, fwant)[0], fwant, "%s/%s %r on the partner" % (f, fform, fargs))
                self.cur_table = s.view
        # the pointers handed out earlier: those the ledger ends are dropped unread, the others must still read the same
        payload = None
        if spec:
            payload = {p: (sp, self._read(sp)) for p, sp in spec.items()}       # (the host copy taken right after the call: the arrays as they lie there)
        mine = set(payload or ())
        for p in self.held.apply(s, self.trim_calls, payload):
            if p in mine and self.held.live[p][0] == s.idx:
                continue
            sp, copy = self.held.live[p][1]
            self.n_reread += 1
            self.compare(s, self._read(sp), copy, "the %s result of step %d, still valid by the header, read again" % (p, self.held.live[p][0]))
        # the view: the same pointers, the same bytes
        if s.view is not None and rc == 0:
            ptrs = self.kc.export_device()
            if self.view_ptrs is None:
                self.view_ptrs, self.view_copy = ptrs, self._read(self._triple(ptrs, ptrs[3]))
                self.compare(s, self.view_copy, self.m.expected(s.view, "export", ()), "the view")
            elif ptrs != self.view_ptrs:
                self._fail(s, "kmc_export_device returns %r, the view was at %r" % (ptrs, self.view_ptrs))
            else:
                self.compare(s, self._read(self._triple(ptrs, ptrs[3])), self.view_copy, "the view's bytes")

    def _sizes_of_nothing(self, s):
        """what the host forms that take their sizes from the expected value get when an error is expected: no entries"""
        z = np.zeros(0, U64)
        return {n: z for n in ("segs", "support", "verdict", "link_support", "transit_count", "cands")}

    def walk(self, n_steps=None):
        for s in self.steps[:n_steps]:
            self.step(s)


def child_main(argv):
    """the trace cases: python -c 'import view_runner, sys; view_runner.child_main(sys.argv)' ROOT k canonical seed n_steps"""
    import importlib
    root, k, canonical, seed, n_steps = argv[1], int(argv[2]), argv[3] == "1", int(argv[4]), int(argv[5])
    sys.path.insert(0, root)
    kmc = importlib.import_module("k-mer-count_amd")
    steps = vs.sequence(k, canonical, seed)
    r = Runner(kmc, vx.Menu(k, canonical), k, canonical, seed, steps, mark=lambda text: print("@ " + text, file=sys.stderr, flush=True))
    try:
        r.walk(n_steps)
    finally:
        r.close()
    print("@ end", file=sys.stderr, flush=True)
