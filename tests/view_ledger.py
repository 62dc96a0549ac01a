"""The state rules include/kmc.h gives the calls that read the sorted view, restated as a host model (no GPU, no library).

One Ledger follows one ctx call by call and says, from the header's words alone, what each call must do:

  * which results the ctx HOLDS afterwards and for which (view, range, limits) -- unitigs, links, the map row index, the
    clean / simplify, components, bubbles and transits results -- and so whether a call computes or copies: the "Cost:" notes
    and the "RELATION TO THE OTHER VIEW CALLS" paragraphs;
  * the KMC_UNITIG_TRACE lines a call that computes prints, with their unitigs_reused / links_reused flags;
  * the return code: KMC_OK, or KMC_ERR_STATE without a view and for a KMC_TRANSIT_ACCUMULATE with nothing to add to;
  * for every family of device pointers the ABI hands out, which later calls END its validity: the "valid until the next
    ..." sentence of each device form.  Where the header says nothing about a pair the ledger says "ended": a test must
    never read through a pointer the header does not promise.  SILENT lists those pairs.

The unit is one ABI call (Ledger.call); a test step is a short fixed series of them (EXPANSION): a host form that sizes
first and copies second is two calls, the second of which finds the first one's result held.  The source is the header,
not kmc_views.hip; tests/test_view_sequences_host.py checks the ledger against the orderings the trace tests pin."""

OK, ERR_STATE = 0, -9

FAMILIES = ("export", "partition", "histogram", "filter", "query", "profile", "compare", "graph", "unitigs", "links", "map",
            "transits", "correct", "trim", "normalize", "clean", "simplify", "components", "bubbles", "into")
# the families with a device form of their own (kmc_*_device); the others have the host form alone
DEVICE_FORMS = frozenset(FAMILIES) - {"histogram", "into"}
HOST_FORMS = frozenset(FAMILIES) - {"partition"}

PRODUCERS = ("fresh", "async", "double", "refinalize", "empty", "none", "merge")

POINTERS = ("view", "partition", "filter", "setop", "adj", "unitig_arrays", "link_arrays", "map_arrays", "correct_arrays",
            "trim_arrays", "trim_double", "normalize_arrays", "clean", "components", "bubbles", "transits")

# ABI calls -> (family, form)
CALLS = {
    "export": ("export", "host"), "export_device": ("export", "device"), "partition_device": ("partition", "device"),
    "histogram": ("histogram", "host"), "export_filtered": ("filter", "host"), "filter_device": ("filter", "device"),
    "query": ("query", "host"), "query_device": ("query", "device"), "profile": ("profile", "host"),
    "profile_device": ("profile", "device"), "compare": ("compare", "host"), "export_setop": ("compare", "host"),
    "setop_device": ("compare", "device"), "graph": ("graph", "host"), "graph_device": ("graph", "device"),
    "unitigs": ("unitigs", "host"), "unitigs_device": ("unitigs", "device"), "unitig_links": ("links", "host"),
    "unitig_links_device": ("links", "device"), "unitig_map": ("map", "host"), "unitig_map_device": ("map", "device"),
    "unitig_transits": ("transits", "host"), "unitig_transits_device": ("transits", "device"), "correct": ("correct", "host"),
    "correct_device": ("correct", "device"), "trim": ("trim", "host"), "trim_device": ("trim", "device"),
    "normalize": ("normalize", "host"), "normalize_device": ("normalize", "device"), "unitig_clean": ("clean", "host"),
    "unitig_clean_device": ("clean", "device"), "unitig_simplify": ("simplify", "host"),
    "unitig_simplify_device": ("simplify", "device"), "unitig_components": ("components", "host"),
    "unitig_components_device": ("components", "device"), "unitig_bubbles": ("bubbles", "host"),
    "unitig_bubbles_device": ("bubbles", "device"), "unitig_clean_into": ("into", "host"),
    "unitig_simplify_into": ("into", "host"), "unitig_components_into": ("into", "host"),
}

# (family, form) of a test step -> the ABI calls it makes, in order.  The host forms of map, transits and correct are one
# call into arrays sized from the expected result; those of trim and normalize size first and "compute on EVERY call".
EXPANSION = {
    ("export", "host"): ("export_device", "export"), ("export", "device"): ("export_device",),
    ("partition", "device"): ("partition_device",), ("histogram", "host"): ("histogram",),
    ("filter", "host"): ("export_filtered", "export_filtered"), ("filter", "device"): ("filter_device",),
    ("query", "host"): ("query",), ("query", "device"): ("query_device",),
    ("profile", "host"): ("profile",), ("profile", "device"): ("profile_device",),
    ("graph", "host"): ("export_device", "graph"), ("graph", "device"): ("graph_device",),
    ("unitigs", "host"): ("unitigs", "unitigs"), ("unitigs", "device"): ("unitigs_device",),
    ("links", "host"): ("unitig_links", "unitig_links"), ("links", "device"): ("unitig_links_device",),
    ("map", "host"): ("unitig_map",), ("map", "device"): ("unitig_map_device",),
    ("transits", "host"): ("unitig_transits",), ("transits", "device"): ("unitig_transits_device",),
    ("correct", "host"): ("correct",), ("correct", "device"): ("correct_device",),
    ("trim", "host"): ("trim", "trim"), ("trim", "device"): ("trim_device",),
    ("normalize", "host"): ("normalize", "normalize"), ("normalize", "device"): ("normalize_device",),
    ("clean", "host"): ("unitig_clean", "unitig_clean"), ("clean", "device"): ("unitig_clean_device",),
    ("simplify", "host"): ("unitig_simplify", "unitig_simplify"), ("simplify", "device"): ("unitig_simplify_device",),
    ("components", "host"): ("unitig_components", "unitig_components"), ("components", "device"): ("unitig_components_device",),
    ("bubbles", "host"): ("unitig_bubbles", "unitig_bubbles"), ("bubbles", "device"): ("unitig_bubbles_device",),
}

# The pointer family each device form hands out.
GRANTS = {
    "export_device": ("view",), "partition_device": ("partition",), "filter_device": ("filter",), "setop_device": ("setop",),
    "graph_device": ("adj",), "unitigs_device": ("unitig_arrays",), "unitig_links_device": ("link_arrays",),
    "unitig_map_device": ("map_arrays",), "unitig_transits_device": ("transits",), "correct_device": ("correct_arrays",),
    "trim_device": ("trim_arrays", "trim_double"), "normalize_device": ("normalize_arrays",),
    "unitig_clean_device": ("clean",), "unitig_simplify_device": ("clean",), "unitig_components_device": ("components",),
    "unitig_bubbles_device": ("bubbles",),
}

# "valid until the next ... call / finalize / reset / destroy", one entry per pointer family: the families whose calls (either
# form) end it, and the classes of call that do.  A class event is raised by the family itself and by every call that
# "counts as" one because it computes that stage again:
#   unitigs*   a kmc_unitigs* call; a links, map, transits, clean, simplify, components, bubbles or *_into call that
#              computes the unitigs ("counts as a kmc_unitigs* call")
#   links*     a kmc_unitig_links* call; a transits, clean, ... call that computes the links ("counts as a kmc_unitig_links* call")
#   graph*     a kmc_graph* call; whatever computes the unitigs ("kmc_unitigs* counts as a kmc_graph* call ... whenever it computes")
# Every producer (finalize, reset) ends every family.
ENDERS = {
    "view": ((), ()),                                       # "valid until the next finalize/reset/destroy"
    "partition": (("partition",), ()),                      # "Pointers as in kmc_export_device"
    "filter": (("filter",), ()),                            # "the next kmc_filter_device / kmc_export_filtered"
    "setop": (("compare",), ()),                            # "the next set operation"
    "adj": (("graph", "unitigs"), ("graph*", "unitigs*")),  # "the next kmc_graph* or kmc_unitigs* call"
    "unitig_arrays": (("unitigs",), ("unitigs*",)),         # "the next kmc_unitigs* call"
    "link_arrays": (("links", "unitigs", "graph"), ("links*", "unitigs*", "graph*")),
    "map_arrays": (("map", "transits", "unitigs", "graph"), ("unitigs*", "graph*")),   # transits: "map arrays handed out earlier are invalid"
    "correct_arrays": (("correct",), ()),
    "trim_arrays": (("trim",), ()),
    "trim_double": ((), ()),                                # two kmc_trim* calls: Ledger counts them
    "normalize_arrays": (("normalize",), ()),
    "clean": (("clean", "simplify", "into", "links", "unitigs", "graph"), ("links*", "unitigs*", "graph*")),
    "components": (("components", "into", "links", "unitigs", "graph"), ("links*", "unitigs*", "graph*")),
    "bubbles": (("bubbles", "links", "unitigs", "graph"), ("links*", "unitigs*", "graph*")),
    "transits": (("transits", "unitigs", "links", "graph"), ("links*", "unitigs*", "graph*")),
}

# Pairs the header leaves open, which the ledger therefore ends (a later change of kmc.h can settle them):
SILENT = (
    ("partition", "partition", "the partition's pointers are 'as in kmc_export_device'; a second kmc_partition_device is not mentioned"),
    ("setop", "compare", "'the next set operation': whether kmc_compare, which hands out no arrays, is one is not said"),
    ("clean", "into", "kmc_unitig_components_into is not among the enders of a clean result, kmc_unitig_clean_into is by 'kmc_unitig_clean*'"),
    ("components", "into", "the same the other way round: kmc_unitig_clean_into against a components result"),
    ("transits", "unitigs", "'... call that computes': a kmc_unitigs host call that copies is taken as one all the same"),
    ("trim_double", "trim", "the host form kmc_trim is taken to flip the double buffer like kmc_trim_device ('computes on EVERY call')"),
    ("*", "empty view", "what a call on an empty view prints under KMC_UNITIG_TRACE is not said: no trace is predicted there"),
)


class Outcome:
    """What one ABI call must do: rc, the trace lines of what it computes (None: the header does not say), and the
    pointer families its call ends / hands out."""

    def __init__(self, rc, trace=(), ended=(), granted=()):
        self.rc, self.trace, self.ended, self.granted = rc, (None if trace is None else list(trace)), set(ended), tuple(granted)

    def __repr__(self):
        return "Outcome(rc=%d, trace=%r, ended=%r, granted=%r)" % (self.rc, self.trace, sorted(self.ended), self.granted)


class Ledger:
    def __init__(self):
        self.gen = 0                 # counts the views
        self.view = None             # None: no view; else {"empty": bool}
        self._forget()
        self.trim_calls = 0          # kmc_trim* calls so far: a trim_double grant of call i lives while trim_calls <= i + 1

    def _forget(self):
        """finalize / reset: every held result goes"""
        self.u = None                # (range) of the held unitigs
        self.u_live = False          # no kmc_graph* call has rewritten their work arrays
        self.l = None                # (range) of the held links
        self.m_idx = False           # the map row index of the held unitigs is built
        self.cl = self.cc = self.bb = None   # (range, limits) of the held clean / components / bubbles result
        self.tx = None               # (range) of the held transits
        self.tx_batches = []         # the batches added to them

    # ---- producers ----
    def produce(self, kind, empty=False):
        """a new view (empty: it holds no key), or none for kind 'none'; ends every pointer family.  'refinalize' on a view:
        "a call that finds nothing added, merged or reset since the last finalize makes NO new view" (the tables of these
        tests all go the small-table way) -- nothing is dropped and nothing ends"""
        assert kind in PRODUCERS
        if kind == "refinalize" and self.view is not None:
            return Outcome(OK, (), ())
        self._forget()
        if kind == "none":
            self.view = None
        else:
            self.gen += 1
            self.view = {"empty": bool(empty) or kind == "empty"}
        return Outcome(OK, (), POINTERS)

    # ---- stages ----
    def _unitigs(self, rng, ev, trace):
        """the unitigs of this range are needed by a call that "counts as a kmc_unitigs* call": True if they are reused"""
        if self.u == rng and self.u_live:
            return True
        trace.append("kmc_unitigs")
        ev.update(("unitigs*", "graph*"))
        self.u, self.u_live, self.m_idx = rng, True, False
        self.l = self.cc = self.bb = self.tx = None      # "whatever drops the links drops" components, bubbles; transits: "any call that recomputes the unitigs or the links"
        self.tx_batches = []
        return False

    def _links(self, rng, ev, trace, may_copy):
        """the links of this range: copied (kmc_unitig_links), reused (a clean, components, bubbles or transits call, "under
        the condition of a clean call": unitigs held and their work arrays not rewritten) or computed.  True if not computed."""
        if may_copy and self.l == rng:
            return True
        if self.l == rng and self.u == rng and self.u_live:
            return True
        reused = self._unitigs(rng, ev, trace)
        trace.append("kmc_unitig_links unitigs_reused %d" % reused)
        ev.add("links*")
        self.l = rng
        self.cc = self.bb = self.tx = None
        self.tx_batches = []
        return False

    # ---- one ABI call ----
    def call(self, name, rng=None, limits=None, accumulate=False, batch=None):
        """name: a key of CALLS; rng: (min_count, max_count) of the graph families; limits: the tuple of limits of a clean
        (tip, island), simplify (tip, island, bubble), components or bubbles (limit,) call; accumulate / batch: transits"""
        family, form = CALLS[name]
        if self.view is None:
            return Outcome(ERR_STATE)            # "no view: KMC_ERR_STATE"; nothing is changed
        trace, ev = [], set()
        if family == "graph":
            self.u_live = self.m_idx = False     # "anything that rewrites adj": the next links, map or transits call recomputes the unitigs
            self.tx, self.tx_batches = None, []  # "a kmc_graph* call in between makes the next transits call one of those"
            ev.add("graph*")
        elif family == "unitigs":
            ev.add("unitigs*")
            if form == "device" or self.u != rng:    # "kmc_unitigs_device always computes"; the host form copies what is held
                self.u = None
                self._unitigs(rng, ev, trace)
        elif family == "links":
            ev.add("links*")
            if form == "device":                      # "Always computes the links pass"
                self.l = None
            self._links(rng, ev, trace, may_copy=form == "host")
        elif family == "map":
            reused = self._unitigs(rng, ev, trace)
            self.m_idx = True                         # "built once per unitig result and dropped with it"
            trace.append("kmc_unitig_map unitigs_reused %d" % reused)
        elif family == "transits":
            if accumulate and not (self.tx == rng and self.l == rng and self.u == rng and self.u_live):
                return Outcome(ERR_STATE)             # "No such result held: KMC_ERR_STATE"
            reused = self._links(rng, ev, trace, may_copy=False)
            if not accumulate:
                self.tx_batches = []
            trace.append("kmc_unitig_map unitigs_reused 1")     # "Links first, then map, then the transit passes"
            self.m_idx = True
            trace.append("kmc_unitig_transits links_reused %d" % reused)
            self.tx = rng
            self.tx_batches = self.tx_batches + [batch]
        elif family in ("correct", "trim", "normalize"):
            trace.append("kmc_" + family)             # "computes on EVERY call"
            if family == "trim":
                self.trim_calls += 1
        elif family in ("clean", "simplify") or name in ("unitig_clean_into", "unitig_simplify_into"):
            key = (rng,) + tuple(limits) + ((0,) if len(limits) == 2 else ())       # "a clean call having bubble limit 0"
            if not (form == "host" and family != "into" and self.cl == key):
                self._links(rng, ev, trace, may_copy=False)
                trace.append("kmc_unitig_simplify" if "simplify" in name else "kmc_unitig_clean")
                self.cl = key
        elif family == "components" or name == "unitig_components_into":
            key = (rng,) + tuple(limits)
            if not (form == "host" and family != "into" and self.cc == key):
                self._links(rng, ev, trace, may_copy=False)
                trace.append("kmc_unitig_components")
                self.cc = key
        elif family == "bubbles":
            key = (rng,) + tuple(limits)
            if not (form == "host" and self.bb == key):
                self._links(rng, ev, trace, may_copy=False)
                trace.append("kmc_unitig_bubbles")
                self.bb = key
        ended = {p for p, (fams, classes) in ENDERS.items() if family in fams or ev & set(classes)}
        return Outcome(OK, None if self.view["empty"] else trace, ended, GRANTS.get(name, ()))

    def double_alive(self, born):
        """a trim_double grant made when trim_calls was `born`: "the result of the call BEFORE the last one is gone\""""
        return self.trim_calls - born <= 1

    def step(self, family, form, names=None, **args):
        """a test step: the Outcomes of its ABI calls (EXPANSION; a compare or *_into step names its calls)"""
        names = names or EXPANSION[(family, form)]
        return [self.call(n, **(args if CALLS[n][0] == family else {})) for n in names]


def merged(outcomes):
    """one Outcome for a step: the first error, else the traces in order, everything ended, the last grants"""
    for o in outcomes:
        if o.rc:
            return o
    trace = None if any(o.trace is None for o in outcomes) else [t for o in outcomes for t in o.trace]
    return Outcome(OK, trace, set().union(*[o.ended for o in outcomes]), outcomes[-1].granted)
