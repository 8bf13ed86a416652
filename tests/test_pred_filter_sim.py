"""The predecessor filter's flags are complete (CPU, tools/sim): on the small
graphs of tests/plan_cost_cases.py and the quantised ba1200, with the engine's
own batches (pe_plan.cpp, batch order 2) at 8 and 16 lanes, the simulator's
relax flags an arc when some active lane's pre-check finds du + w <= dist[x];
every arc that is tight in any lane's final distances must be flagged, and no
unflagged arc may undercut its head.  The quantised graph (equal-length
alternatives: relaxations that find du + w == dist[x] and improve nothing) is
the one that fails if the test is `<` instead of `<=`."""
import os
import sys

import numpy as np
import pytest

from plan_cost_cases import plan_cost_graphs
from shdpe import generators as G

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "sim"))
import pred_filter_eval as pf  # noqa: E402


def _cases():
    c = {name: (top, np.asarray(att, np.int32)) for name, top, att in plan_cost_graphs()}
    c["ba1200q"] = (G.power_law(1200, m=3, seed=4, quantum=0.005), G.sample_attached(1200, 300, seed=2).astype(np.int32))
    return c


CASES = _cases()


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("pred_filter_sim"))
    return pf.plan_lib(d), pf.sim_lib(d)


@pytest.mark.parametrize("lanes", [8, 16])
@pytest.mark.parametrize("case", list(CASES))
def test_every_tight_arc_is_flagged(libs, case, lanes):
    L, S = libs
    top, att = CASES[case]
    plan = pf.make_plan(L, top, att, lanes)
    tightArcs = equalOnly = 0
    for b in range(plan["srcs"].shape[0]):
        flag, D = pf.relax_batch(S, plan, b)
        tight, under = pf.arc_classes(plan, D)
        assert not under.any(), (case, lanes, b, "the simulated relax left a Bellman violation")
        missed = np.flatnonzero(tight & (flag == 0))
        assert missed.size == 0, (case, lanes, b, "tight arcs not flagged", missed[:5])
        assert not (under & (flag == 0)).any(), (case, lanes, b)
        tightArcs += int(tight.sum())
        assert flag.sum() < flag.shape[0], (case, lanes, b, "every arc flagged: the flags filter nothing")
    assert tightArcs > 0
