"""Random call sequences over every family of calls that reads the sorted view, on one ctx with a partner ctx (GPU).

The per-family tests start every ordering from a fresh ctx; here some five hundred calls share one: the prefix index, the
compaction scratch, adj, the unitig work arrays, the eight "is this result still that of this view and range" facts and
buffers that only ever grow, so that a small view behind a large one runs on stale bytes.  tests/view_sequences.py builds
the sequences (every ordered pair of families adjacent on one view; every family first behind every kind of producer),
tests/view_ledger.py says from include/kmc.h alone what every call must return, compute and leave valid,
tests/view_expected.py has the models' results and tests/view_runner.py walks a sequence and checks every step.
tests/test_view_sequences_host.py checks those four without a GPU."""
import os
import subprocess
import sys

import pytest

import view_expected as vx
import view_runner
import view_sequences as vs
from conftest import ROOT

pytestmark = pytest.mark.gpu

_menus = {}


def _menu(k, canonical):
    """the tables, batches and memoised expected values of a configuration, shared by its cases and left unchanged"""
    if (k, canonical) not in _menus:
        _menus[(k, canonical)] = vx.Menu(k, canonical)
    return _menus[(k, canonical)]


@pytest.mark.parametrize("seed", vs.SEEDS)
@pytest.mark.parametrize("k,canonical", vx.CONFIGS)
def test_view_call_sequences(kmc, k, canonical, seed):
    steps = vs.sequence(k, canonical, seed)
    r = view_runner.Runner(kmc, _menu(k, canonical), k, canonical, seed, steps)
    try:
        r.walk()
    finally:
        r.close()
    assert r.n_results == sum(1 for s in steps if s.kind == "call" and s.outcome.rc == 0) >= 400 and r.n_reread >= 500


_CHILD = "import sys; sys.path.insert(0, sys.argv[6]); import view_runner; view_runner.child_main(sys.argv)"


def _line(text):
    """a KMC_UNITIG_TRACE line as the ledger writes it: the name, and the reuse flag of the three lines that carry one"""
    name = text.split(":")[0]
    flag = {"kmc_unitig_links": "unitigs_reused", "kmc_unitig_map": "unitigs_reused", "kmc_unitig_transits": "links_reused"}.get(name)
    return name if flag is None else "%s %s %s" % (name, flag, text.split(flag + " ")[1].split()[0])


@pytest.mark.parametrize("k,canonical", vx.CONFIGS)
def test_what_computes_through_the_trace_lines(kmc, k, canonical):
    """The first steps of a sequence in a child process with KMC_UNITIG_TRACE set: per step the kmc_* lines on stderr, with
    their unitigs_reused / links_reused flags, are the ledger's prediction of what computes and what is copied (nothing is
    timed).  The child checks every result as the cases above do."""
    seed = vs.SEEDS[0]
    steps = vs.sequence(k, canonical, seed)[:vs.TRACE_STEPS]
    env = dict(os.environ, KMC_UNITIG_TRACE="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(k), "1" if canonical else "0", str(seed), str(vs.TRACE_STEPS),
                        os.path.dirname(os.path.abspath(__file__))], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    seen, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("@ "):
            cur = int(line.split()[2]) if line.startswith("@ step ") else None
            if cur is not None:
                seen[cur] = []
        elif line.startswith("kmc_") and cur is not None:
            seen[cur].append(_line(line))
    assert "@ end" in r.stderr
    checked = 0
    for s in steps:
        if s.kind != "call" or s.outcome.trace is None:
            continue
        last = "\n".join(x.text() for x in steps[max(0, s.idx - 9):s.idx + 1])
        assert seen.get(s.idx) == s.outcome.trace, "k=%d canonical=%s seed=%d step %d prints %r, the ledger says %r\n%s" % (
            k, canonical, seed, s.idx, seen.get(s.idx), s.outcome.trace, last)
        checked += 1
    assert checked >= 80
