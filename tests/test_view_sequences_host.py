"""CPU checks of what tests/test_view_sequences_gpu.py stands on: the ledger (view_ledger.py) against the orderings the
per-family trace tests pin, the conditions the generated sequences (view_sequences.py) must meet -- conditions, not
measurements: the seeds are chosen so that they hold -- and the models' answers for every entry of the menu
(view_expected.py), whose tables are held against the CPU oracle's."""
import numpy as np
import pytest

import map_inputs as mi
import view_expected as vx
import view_ledger as vl
import view_sequences as vs

K = 31


def _ledger():
    g = vl.Ledger()
    g.produce("fresh")
    return g


def _names(trace):
    """the trace lines as the per-family tests write them: the name, ' reused' behind a line that says it reused"""
    return [t.split()[0] + (" reused" if t.endswith("reused 1") else "") for t in trace]


def _do(g, family, form="host", **args):
    o = vl.merged(g.step(family, form, **args))
    assert o.rc == vl.OK
    return o.trace


def test_links_after_unitigs_compute_the_unitigs_once():
    """test_links_gpu.py"""
    g = _ledger()
    assert _names(_do(g, "unitigs", rng=(1, 0))) == ["kmc_unitigs"]
    assert _names(_do(g, "links", rng=(1, 0))) == ["kmc_unitig_links reused"]
    assert _do(g, "links", rng=(1, 0)) == []
    assert _names(_do(g, "links", "device", rng=(1, 0))) == ["kmc_unitig_links reused"]
    _do(g, "graph")
    assert _do(g, "links", rng=(1, 0)) == []                       # the held links are copied: a graph call rewrites adj, not them
    assert _names(_do(g, "links", rng=(2, 0))) == ["kmc_unitigs", "kmc_unitig_links"]


def test_orderings_through_the_trace_lines():
    """test_transits_gpu.py: the transit line carries links_reused, the map line in front of it unitigs_reused"""
    g = _ledger()
    assert _names(_do(g, "unitigs", rng=(1, 0)) + _do(g, "links", rng=(1, 0))) == ["kmc_unitigs", "kmc_unitig_links reused"]
    t = lambda **a: _do(g, "transits", "device", rng=(1, 0), batch=0, **a)
    assert t() == ["kmc_unitig_map unitigs_reused 1", "kmc_unitig_transits links_reused 1"]
    assert _do(g, "unitigs", rng=(1, 0)) == [] and _names(_do(g, "map", "device", rng=(1, 0))) == ["kmc_unitig_map reused"]
    _do(g, "graph")
    assert t() == ["kmc_unitigs", "kmc_unitig_links unitigs_reused 0", "kmc_unitig_map unitigs_reused 1", "kmc_unitig_transits links_reused 0"]
    assert _do(g, "clean", rng=(1, 0), limits=(K, K)) == ["kmc_unitig_clean"]
    assert _do(g, "bubbles", rng=(1, 0), limits=(K,)) == ["kmc_unitig_bubbles"]
    assert t() == ["kmc_unitig_map unitigs_reused 1", "kmc_unitig_transits links_reused 1"]       # clean and bubbles: copied, not computed
    assert _do(g, "clean", rng=(1, 0), limits=(K, K)) == [] and _do(g, "bubbles", rng=(1, 0), limits=(K,)) == []


def test_map_clean_simplify_components_and_bubbles_reuse():
    """test_map_gpu.py, test_clean_gpu.py, test_simplify_gpu.py, test_components_gpu.py, test_bubble_calls_gpu.py"""
    g = _ledger()
    assert _names(_do(g, "unitigs", rng=(1, 0))) == ["kmc_unitigs"]
    assert _names(_do(g, "map", "device", rng=(1, 0))) == ["kmc_unitig_map reused"]
    _do(g, "graph")
    assert _names(_do(g, "map", "device", rng=(1, 0))) == ["kmc_unitigs", "kmc_unitig_map"]
    _do(g, "links", rng=(1, 0))
    assert _names(_do(g, "map", "device", rng=(1, 0))) == ["kmc_unitig_map reused"]
    _do(g, "clean", rng=(1, 0), limits=(K, K))
    assert _names(_do(g, "map", "device", rng=(1, 0))) == ["kmc_unitig_map reused"]

    g = _ledger()
    first = lambda trace: [t.split()[0] for t in trace]
    c = lambda form="host", rng=(1, 0), limits=(K, K): first(_do(g, "clean", form, rng=rng, limits=limits))
    assert first(_do(g, "links", rng=(1, 0))) == ["kmc_unitigs", "kmc_unitig_links"]
    assert c() == ["kmc_unitig_clean"] and c() == [] and c(limits=(5, 5)) == ["kmc_unitig_clean"] and c("device") == ["kmc_unitig_clean"]
    _do(g, "graph")
    assert c("device") == ["kmc_unitigs", "kmc_unitig_links", "kmc_unitig_clean"]
    assert c(rng=(2, 0)) == ["kmc_unitigs", "kmc_unitig_links", "kmc_unitig_clean"]

    g = _ledger()
    s = lambda form="host", rng=(1, 0), limits=(K, K, K): first(_do(g, "simplify", form, rng=rng, limits=limits))
    _do(g, "links", rng=(1, 0))
    assert s() == ["kmc_unitig_simplify"] and s() == []
    assert c() == ["kmc_unitig_clean"] and s() == ["kmc_unitig_simplify"] and s(limits=(K, K, 5)) == ["kmc_unitig_simplify"]
    assert s(limits=(K, K, 0)) == ["kmc_unitig_simplify"] and c() == []            # a simplify with limit 0 and a clean share one result
    assert s("device") == ["kmc_unitig_simplify"]
    _do(g, "graph")
    assert s() == [] and s("device") == ["kmc_unitigs", "kmc_unitig_links", "kmc_unitig_simplify"]     # the held result is copied; the pass finds adj rewritten

    for family, line, limits, other in (("components", "kmc_unitig_components", (K,), (3,)), ("bubbles", "kmc_unitig_bubbles", (K,), (5,))):
        g = _ledger()
        p = lambda form="host", rng=(1, 0), limits=limits: _do(g, family, form, rng=rng, limits=limits)
        assert _do(g, "links", rng=(1, 0)) == ["kmc_unitigs", "kmc_unitig_links unitigs_reused 0"]
        assert p() == [line] and p() == [] and p(limits=other) == [line]
        assert first(_do(g, "clean", rng=(1, 0), limits=(K, K)) + _do(g, "simplify", rng=(1, 0), limits=(K, K, K))) == ["kmc_unitig_clean", "kmc_unitig_simplify"]
        assert p(limits=other) == [] and p("device") == [line]
        assert _do(g, "links", "device", rng=(1, 0)) + p() == ["kmc_unitig_links unitigs_reused 1", line]       # the links pass drops the result
        _do(g, "graph")
        assert p() == [] and p("device") == ["kmc_unitigs", "kmc_unitig_links unitigs_reused 0", line]
        assert _do(g, "unitigs", rng=(3, 0)) + p(rng=(3, 0)) == ["kmc_unitigs", "kmc_unitig_links unitigs_reused 1", line]
        g.produce("refinalize")
        assert p(rng=(3, 0)) == []                                                                               # nothing added: no new view
        g.produce("double")
        assert p(rng=(3, 0)) == ["kmc_unitigs", "kmc_unitig_links unitigs_reused 0", line]                       # a new view


def test_state_errors_and_accumulate():
    g = vl.Ledger()
    for name in vl.CALLS:
        assert g.call(name, rng=(1, 0), limits=(1, 1)).rc == vl.ERR_STATE         # no view yet
    g.produce("fresh")
    acc = lambda rng=(1, 0): g.call("unitig_transits_device", rng=rng, accumulate=True, batch=1).rc
    assert acc() == vl.ERR_STATE                                                  # nothing held
    assert g.call("unitig_transits_device", rng=(1, 0), batch=0).rc == vl.OK and acc() == vl.OK and g.tx_batches == [0, 1]
    for name in ("unitig_map_device", "correct", "trim", "normalize", "profile", "query", "unitig_bubbles", "unitig_clean"):
        g.call(name, rng=(1, 0), limits=(K, K))
    assert acc() == vl.OK and g.tx_batches == [0, 1, 1] and acc((2, 0)) == vl.ERR_STATE
    g.call("graph")
    assert acc() == vl.ERR_STATE
    assert g.call("unitig_transits", rng=(1, 0), batch=1).rc == vl.OK and g.tx_batches == [1]
    g.call("unitig_links_device", rng=(1, 0))
    assert acc() == vl.ERR_STATE
    g.produce("none")
    assert g.call("export").rc == vl.ERR_STATE and g.produce("empty").rc == vl.OK and g.call("export").rc == vl.OK


def test_pointer_lifetimes():
    g = _ledger()
    assert set(vl.ENDERS) == set(vl.POINTERS) and {p for v in vl.GRANTS.values() for p in v} == set(vl.POINTERS)
    ended = lambda name, **a: g.call(name, **a).ended
    assert ended("export") == set() and ended("query") == set() and ended("histogram") == set()
    assert ended("filter_device") == {"filter"} and ended("export_filtered") == {"filter"} and ended("compare") == {"setop"}
    assert ended("graph") == {"adj", "link_arrays", "map_arrays", "clean", "components", "bubbles", "transits"}
    g.call("unitigs_device", rng=(1, 0))
    g.call("unitig_links_device", rng=(1, 0))
    # a clean call behind the links of its range "rewrites neither of them, nor adj": only a clean result ends
    assert ended("unitig_clean_device", rng=(1, 0), limits=(K, K)) == {"clean"}
    assert ended("unitig_components_device", rng=(1, 0), limits=(K,)) == {"components"}
    assert ended("unitig_bubbles_device", rng=(1, 0), limits=(K,)) == {"bubbles"}
    assert ended("unitig_map_device", rng=(1, 0)) == {"map_arrays"}
    assert ended("unitig_transits_device", rng=(1, 0), batch=0) == {"map_arrays", "transits"}
    assert ended("correct_device") == {"correct_arrays"} and ended("normalize_device") == {"normalize_arrays"}
    # of another range it computes the unitigs and the links again: it counts as a call of each
    assert ended("unitig_clean_device", rng=(2, 0), limits=(K, K)) == set(vl.POINTERS) - {
        "view", "partition", "filter", "setop", "correct_arrays", "trim_arrays", "trim_double", "normalize_arrays"}
    born = g.trim_calls
    assert ended("trim_device") == {"trim_arrays"} and g.double_alive(born) and ended("trim") == {"trim_arrays"} and not g.double_alive(born)
    assert g.produce("refinalize").ended == set() and g.produce("fresh").ended == set(vl.POINTERS)


CASES = [(k, c, s) for k, c in vx.CONFIGS for s in vs.SEEDS]
_SEQ = {}


def _sequence(k, canonical, seed):
    if (k, canonical, seed) not in _SEQ:
        _SEQ[(k, canonical, seed)] = vs.sequence(k, canonical, seed)
    return _SEQ[(k, canonical, seed)]


@pytest.mark.parametrize("k,canonical,seed", CASES)
def test_generator_conditions(k, canonical, seed):
    steps = _sequence(k, canonical, seed)
    assert [s.text() for s in steps] == [s.text() for s in vs.sequence(k, canonical, seed)]       # deterministic
    calls = [s for s in steps if s.kind == "call"]
    # every ordered pair adjacent on one view
    pairs = {(a.name, b.name) for a, b in zip(steps, steps[1:]) if a.kind == b.kind == "call" and a.view is not None}
    assert pairs == {(a, b) for a in vl.FAMILIES for b in vl.FAMILIES}
    # T_big both precedes and follows a smaller table
    tables = [s.view[0] for s in steps if s.kind == "produce" and s.view is not None and s.view[0] in ("few", "mid", "big")]
    first_big, last_big = tables.index("big"), len(tables) - 1 - tables[::-1].index("big")
    assert any(t != "big" for t in tables[:first_big]) and any(t != "big" for t in tables[last_big:])
    assert any(a == "big" and b != "big" for a, b in zip(tables, tables[1:])) and any(a != "big" and b == "big" for a, b in zip(tables, tables[1:]))
    # the empty view and the no-view state, each with five families or more behind them
    assert len({s.name for s in calls if s.view is None}) >= 5 and len({s.name for s in calls if s.view == ("empty", 1)}) >= 5
    assert all((s.outcome.rc == vl.ERR_STATE) == (s.view is None or (s.accumulate and s.outcome.rc != 0)) for s in calls)
    # ACCUMULATE both legally and illegally, on a view
    acc = [s.outcome.rc for s in calls if s.accumulate and s.view is not None]
    assert vl.OK in acc and vl.ERR_STATE in acc
    assert any(len(s.args[1]) >= 2 for s in calls if s.name == "transits")        # ... and a total over two batches or more
    # every device pointer family held across a call that leaves it valid and across one that ends it
    held, stayed, ended = vs.Held(), set(), set()
    for s, n_trim in zip(steps, vs.trim_calls_after(steps)):
        before = set(held.live)
        kept = set(held.apply(s, n_trim))
        if s.kind == "call":
            stayed |= kept
        ended |= before - kept          # (the view's pointers are ended by producers alone)
    assert stayed == set(vl.POINTERS) and ended == set(vl.POINTERS)
    # both forms of every family that has two, every menu entry of the ranges
    assert {(s.name, s.form) for s in calls} == {(f, "host") for f in vl.HOST_FORMS} | {(f, "device") for f in vl.DEVICE_FORMS}
    assert any(s.follow for s in calls) and 450 <= len(calls) <= 700


@pytest.mark.parametrize("k,canonical", vx.CONFIGS)
def test_every_family_first_behind_every_producer(k, canonical):
    seen = {(s.first_behind, s.name) for seed in vs.SEEDS for s in _sequence(k, canonical, seed) if s.kind == "call" and s.first_behind}
    assert seen == {(p, f) for p in vl.PRODUCERS for f in vl.FAMILIES}


_MENUS = {}


def menu(k, canonical):
    if (k, canonical) not in _MENUS:
        _MENUS[(k, canonical)] = vx.Menu(k, canonical)
    return _MENUS[(k, canonical)]


@pytest.mark.parametrize("k,canonical", vx.CONFIGS)
def test_tables_and_batches(oracle, k, canonical):
    import bubble_model as bm
    import chunk_inputs
    import clean_model as cm
    import transit_model as tm
    from test_unitig_gpu import _table_dict
    m = menu(k, canonical)
    sizes = {name: len(m.table((name, 1))) for name in ("few", "mid", "big", "empty")}
    assert 40 <= sizes["few"] <= 80 and 300 <= sizes["mid"] <= 900 and 2049 <= sizes["big"] <= 2600 and sizes["empty"] == 0, sizes
    for name in ("few", "mid", "big"):
        # the CPU oracle's table: the keys, their packing and the counts
        want = oracle.count_kmers(*mi.pack(m.reads[name]), k, canonical)
        assert _table_dict(want) == m.table((name, 1))
        hi, lo, cnt = m.arrays((name, 1))
        assert np.array_equal(hi, want.key_hi) and np.array_equal(lo, want.key_lo) and np.array_equal(cnt, want.count)
        assert all(c == 2 * m.table((name, 1))[x] for x, c in m.table((name, 2)).items())
        # every range has unitigs, and (2, 0) is another solid set once the counts double
        for tid in ((name, 1), (name, 2)):
            assert all(len(m.graph(tid, rng)[0].seqs) > 0 for rng in vx.RANGES), (tid,)
        assert m.graph((name, 1), (2, 0))[0].summary[2] < m.graph((name, 2), (2, 0))[0].summary[2] == sizes[name]
    # the shapes of T_mid: a tip, an island, a bubble, a circular unitig, a repeat with dS, dE >= 2, for even k a palindrome
    mid = m.table(("mid", 1))
    c = cm.clean(mid, canonical, graph=m.graph(("mid", 1), (1, 0)))
    assert c.summary[1] >= 1 and c.summary[2] >= 1
    assert bm.simplify(mid, canonical, graph=m.graph(("mid", 1), (1, 0))).summary[8] >= 1
    u, lk = m.graph(("mid", 1), (1, 0))
    assert u.summary[3] >= 1
    t = tm.Transits(lk, len(u.seqs), k)
    assert any(a >= 2 and b >= 2 for a, b in zip(t.d_start, t.d_end))
    if canonical and k % 2 == 0:
        import graph_model as gm
        assert any(x == gm.revcomp(x) for x in mid)
    a, b = m.batches
    assert len(a) >= 40 and max(map(len, a)) > chunk_inputs.CHUNK and min(map(len, a)) == 0 and len(a) % 2 == 0 and len(b) % 2 == 0
    assert any(ch not in "ACGT" for r in a for ch in r) and sum(map(len, b)) % 2 == 1
    assert max(len(r) for r in a if len(r) <= chunk_inputs.CHUNK) <= 300 + 2 * k + k + 12
    # reads that cross unitig ends of T_mid: crossings in both batches, transits through the repeat in their sum
    for i in (0, 1):
        assert m.expected(("mid", 1), "map", ((1, 0), i))["words"][4] > 0
    assert m.expected(("mid", 1), "transits", ((1, 0), (0, 1), 1))["words"][3] > 0


@pytest.mark.parametrize("k,canonical,seed", CASES)
def test_models_answer_every_step(k, canonical, seed):
    """every (table, arguments) a sequence uses -- the partner's kept tables and the calls on them included -- has an expected
    value; this also warms the memo and bounds the models' time"""
    m = menu(k, canonical)
    n = 0
    for s in _sequence(k, canonical, seed):
        if s.kind != "call" or s.outcome.rc:
            continue
        want = m.expected(s.view, s.name, s.args, s.partner if s.name == "compare" else None)
        assert want and all(isinstance(v, np.ndarray) for v in want.values())
        n += 1
        if s.follow:
            kept = ("kept", s.view) + s.args
            assert m.arrays(kept)[1].shape[0] == int(m.expected(s.view, "into", s.args)["words"][3 if s.args[0] != "components" else 6])
            assert m.expected(kept, s.follow[0], s.follow[2])
    assert n > 400
