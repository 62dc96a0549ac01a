"""Deterministic call sequences over every family of calls that reads the sorted view (no GPU, no library).

sequence(k, canonical, seed) builds one list of Steps for one ctx and a partner ctx:

  * first a shuffled Eulerian circuit of the complete directed graph on the twenty families, self-loops included: every
    ordered pair (A, B) occurs once with B the very next view call after A.  A producer cuts it every 20..30 steps and the
    last family before the cut is repeated as the first call behind it, so the pair that spans the cut is not lost.  These
    producers all give a view with keys (a pair on no view shows nothing);
  * then the tail.  Every family has to come first behind every producer kind over the seeds of a configuration: 7 x 20
    combinations, far more than random cuts would meet.  So the tail takes this seed's share of the shuffled combinations,
    runs producer and family for each and puts up to two uniformly random steps behind it.

Arguments come from the small menus of view_expected.py.  While it builds the sequence the generator runs the Ledger
(view_ledger.py) along: every Step carries the view and the partner's table it runs on and the Outcome the header
predicts -- the return code, the trace lines, the pointer families it ends and hands out -- and a transits step with
KMC_TRANSIT_ACCUMULATE is drawn more often when the ledger says it is legal, so that both cases occur."""
import numpy as np

import view_expected as vx
import view_ledger as vl

SEEDS = (0, 1)
TRACE_STEPS = 120
FOLLOW = tuple(f for f in vl.FAMILIES if f not in ("compare", "into", "partition"))    # what runs on the partner behind a *_into step


class Step:
    def __init__(self, idx, kind, name, form="host", args=(), table=None, phase="euler"):
        self.idx, self.kind, self.name, self.form, self.args, self.table, self.phase = idx, kind, name, form, args, table, phase
        self.names = None          # the ABI calls, where the family alone does not say (compare, into)
        self.ledger_args = {}
        self.view = None           # call: the table the view holds (None: no view); produce: the table it gives
        self.partner = None        # the table the partner's view holds when the step runs
        self.outcome = None
        self.follow = None         # into: (family, form, args) of the further call on the partner
        self.accumulate = False
        self.first_behind = None   # the producer kind right in front of this call

    def text(self):
        if self.kind == "produce":
            return "%03d produce %s(%s) -> %s" % (self.idx, self.name, self.table or "", self.view)
        acc = " ACCUMULATE" if self.accumulate else ""
        return "%03d %s/%s%s %r on %s, partner %s -> rc %d" % (self.idx, self.name, self.form, acc, self.args, self.view, self.partner,
                                                               self.outcome.rc)


def euler_circuit(rng, n):
    """a closed walk over every ordered pair of 0..n-1 exactly once, loops included (Hierholzer, shuffled)"""
    out = [list(rng.permutation(n)) for _ in range(n)]
    stack, walk = [int(rng.integers(0, n))], []
    while stack:
        v = stack[-1]
        if out[v]:
            stack.append(int(out[v].pop()))
        else:
            walk.append(stack.pop())
    walk.reverse()
    assert len(walk) == n * n + 1 and len(set(zip(walk, walk[1:]))) == n * n
    return walk


class _Builder:
    def __init__(self, k, canonical, seed):
        self.k, self.canonical = k, canonical
        self.rng = np.random.default_rng([k, seed, 77])
        self.ledger = vl.Ledger()
        self.steps = []
        self.content = None            # what the count table holds: a table name or None (nothing)
        self.view = None
        self.partner = ("few", 1)
        self.tables = ["mid", "big", "few", "big", "mid", "few"]
        self.kinds = [str(x) for x in self.rng.permutation(["fresh", "async", "merge", "double", "refinalize"])]
        self.n_prod = 0
        self.last_producer = None
        self.acc_seen = [False, False]       # an ACCUMULATE has been drawn: legally, illegally

    def pick(self, menu):
        return menu[int(self.rng.integers(0, len(menu)))]

    # ---- producers ----
    def produce(self, kind, phase, table=None):
        if table is None and kind in ("fresh", "async", "merge", "double"):
            table = self.tables[self.n_prod % len(self.tables)]
            if kind == "double" and table == "big":
                table = "mid"
        self.n_prod += 1
        s = Step(len(self.steps), "produce", kind, table=table, phase=phase)
        s.partner = self.partner
        if kind in ("fresh", "async", "merge"):
            self.content = self.view = (table, 1)
            if kind == "merge":
                self.partner = (table, 1)
        elif kind == "double":
            s.args = (self.content != (table, 1),)      # the table has to be counted once first
            self.content = self.view = (table, 2)
        elif kind == "refinalize":
            self.view = self.content or ("empty", 1)
        elif kind == "empty":
            self.content, self.view = None, ("empty", 1)
        else:
            self.content = self.view = None
        s.view = self.view
        s.outcome = self.ledger.produce(kind, empty=self.view is not None and self.view[0] == "empty")
        self.steps.append(s)
        self.last_producer = kind

    # ---- calls ----
    def arguments(self, family):
        """(form, expected-value arguments, ledger arguments, ABI names or None)"""
        k, r = self.k, self.rng
        form = "device" if family in vl.DEVICE_FORMS and (family not in vl.HOST_FORMS or r.integers(0, 2)) else "host"
        rng = self.pick(vx.RANGES)
        batch = int(r.integers(0, 2))
        if family in ("export", "query"):
            return form, (), {}, None
        if family == "partition":
            return form, (vx.N_PARTS,), {}, None
        if family in ("histogram", "filter", "graph"):
            return form, (rng,), {}, None
        if family == "profile":
            return form, (batch, int(r.integers(1, 3))), {}, None
        if family == "compare":
            variant = self.pick(vx.SETOPS)
            form = "host" if variant[0] == "compare" else form
            names = ("compare",) if variant[0] == "compare" else ("setop_device",) if form == "device" else ("export_setop", "export_setop")
            return form, (variant, self.pick(vx.RANGES[:2]), self.pick(vx.RANGES[:2])), {}, names
        if family in ("unitigs", "links"):
            return form, (rng,), {"rng": rng}, None
        if family in ("map", "correct"):
            return form, (rng, batch), ({"rng": rng} if family == "map" else {}), None
        if family == "transits":
            # ACCUMULATE whenever the ledger holds something to add to; without that, never before the first legal one and
            # always until the first illegal one, so that both occur
            held = self.ledger.tx is not None and self.ledger.u_live and self.view is not None
            acc = held or (self.view is not None and self.acc_seen[0] and (not self.acc_seen[1] or r.random() < 0.25))
            if held:
                rng = self.ledger.tx
            if self.view is not None:
                self.acc_seen[0 if held else 1] |= acc
            return form, (rng, batch, int(r.integers(1, 3))), {"rng": rng, "accumulate": acc, "batch": batch}, None
        if family == "trim":
            return form, (rng, batch, self.pick(vx.TRIM_RULES)), {}, None
        if family == "normalize":
            return form, (batch, self.pick(vx.NORM_RULES)), {}, None
        limits = {"clean": vx.clean_limits, "simplify": vx.simplify_limits, "components": vx.component_limits, "bubbles": vx.bubble_limits}
        if family == "into":
            kind = self.pick(vx.INTO_KINDS)
            lim = self.pick(limits[kind](k))
            return "host", (kind, rng, lim), {"rng": rng, "limits": lim}, ("unitig_%s_into" % kind,)
        lim = self.pick(limits[family](k))
        return form, (rng, lim), {"rng": rng, "limits": lim}, None

    def call(self, family, phase):
        form, args, largs, names = self.arguments(family)
        s = Step(len(self.steps), "call", family, form, args, phase=phase)
        s.names, s.ledger_args, s.view, s.partner = names, largs, self.view, self.partner
        s.accumulate = bool(largs.get("accumulate"))
        s.first_behind, self.last_producer = self.last_producer, None
        s.outcome = vl.merged(self.ledger.step(family, form, names, **largs))
        if family == "transits":
            s.args = (args[0], tuple(self.ledger.tx_batches) if s.outcome.rc == 0 else (), args[2])
        if family == "into" and s.outcome.rc == 0:
            self.partner = ("kept", self.view) + args
            f = self.pick(FOLLOW)
            fform, fargs, flargs, _ = self.arguments(f)
            if f == "transits":
                fargs = (fargs[0], (flargs["batch"],), fargs[2])
            s.follow = (f, fform, fargs)
        self.steps.append(s)


def sequence(k, canonical, seed):
    """the Steps of one case"""
    b = _Builder(k, canonical, seed)
    fam = vl.FAMILIES
    walk = euler_circuit(b.rng, len(fam))
    b.produce("fresh", "euler")
    b.call(fam[walk[0]], "euler")
    since, cut = 1, int(b.rng.integers(20, 31))
    for prev, v in zip(walk, walk[1:]):
        if since >= cut:
            b.produce(b.kinds[b.n_prod % len(b.kinds)], "euler")
            b.call(fam[prev], "euler")
            since, cut = 1, int(b.rng.integers(20, 31))
        b.call(fam[v], "euler")
        since += 1
    combos = [(p, f) for p in vl.PRODUCERS for f in fam]
    order = np.random.default_rng([k, 5]).permutation(len(combos))      # one shuffle per configuration, shared by its seeds
    for i in order[SEEDS.index(seed)::len(SEEDS)]:
        p, f = combos[int(i)]
        b.produce(p, "tail")
        b.call(f, "tail")
        for _ in range(int(b.rng.integers(0, 3))):
            b.call(fam[int(b.rng.integers(0, len(fam)))], "tail")
    b.produce("fresh", "tail", "few")             # the big table's buffers, once more under a small table
    for f in ("unitigs", "links", "transits", "transits", "components", "bubbles", "simplify", "filter", "compare", "export"):
        b.call(f, "tail")
    return b.steps


class Held:
    """The device results handed out and not yet ended, by the ledger's word: {pointer family: (step index, payload)}.  One
    grant per family is kept, the latest."""

    def __init__(self):
        self.live = {}

    def apply(self, step, ledger_trim_calls, payloads=None):
        """after a step: drop what it ended, then take what it granted (payloads: {pointer family: anything}).  Returns the
        families that were held across the step and stay valid."""
        o = step.outcome
        if o.rc:
            return sorted(self.live)
        for p in o.ended:
            self.live.pop(p, None)
        if "trim_double" in self.live and ledger_trim_calls - self.live["trim_double"][2] > 1:
            del self.live["trim_double"]
        kept = sorted(self.live)
        for p in (o.granted if step.kind == "call" and step.form == "device" else ()):
            self.live[p] = (step.idx, (payloads or {}).get(p), ledger_trim_calls)
        return kept


def trim_calls_after(steps):
    """per step the number of kmc_trim* calls made up to and including it (what Ledger.trim_calls says)"""
    out, n = [], 0
    for s in steps:
        if s.kind == "call" and s.name == "trim" and s.outcome.rc == 0:
            n += len(vl.EXPANSION[("trim", s.form)])
        out.append(n)
    return out
