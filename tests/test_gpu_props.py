"""GPU tests of the graph property check's device form (shd_pe_graph_props,
pe_props.hip): every field and the membership equal the host form and the
scipy / numpy references of tests/props_cases.py, on every case."""
import ctypes as C
import functools

import numpy as np
import pytest

import props_cases as PC
from shdpe import engine as E

pytestmark = pytest.mark.gpu

CASES = list(PC.cases())


@functools.lru_cache(maxsize=None)
def device_props(name):
    """The device form's answer for a case, computed once.  The budget is far
    above any case's sweeps (the longest: 250 trims of the 500-chain), so no
    answer here comes from the host form whatever the default budget is."""
    return E.graph_props(PC.cases()[name], device=0, sweep_budget=100_000, membership=True)


@pytest.mark.parametrize("name", CASES)
def test_device_form_matches_host_and_scipy(name):
    top = PC.cases()[name]
    got = device_props(name)
    assert got["info"]["handedOff"] == 0, got["info"]         # the device's own answer
    assert got["info"]["sweeps"] >= 1
    PC.assert_props(got, PC.expected(name), name)
    host = E.graph_props(top, membership=True)
    PC.assert_props(got, host, name)
    # without a membership array
    PC.assert_props(E.graph_props(top, device=0), PC.expected(name), name)


def test_plain_count_kernel_gives_the_same_counts(monkeypatch):
    """k_props_count<false> (one atomic per edge; SHDPE_PROPS_COUNT=plain, the
    form tools/props_time.py compares) on the cases the counts decide."""
    monkeypatch.setenv("SHDPE_PROPS_COUNT", "plain")
    for name in ("u_selfloops_parallel", "complete65_u", "complete65_d_minus_edge", "size5000_u"):
        PC.assert_props(E.graph_props(PC.cases()[name], device=0, membership=True), PC.expected(name), name)


@pytest.mark.parametrize("name", CASES)
def test_complete_agrees_with_engine(name):
    top = PC.cases()[name]
    try:
        eng = E.Engine(top, np.arange(min(top.n, 4), dtype=np.int32), device=0)
    except E.EngineError as err:
        assert err.code == E.EINVAL, err                      # a graph shd_pe_create refuses
        assert top.m == 0, name                               # only the edgeless ones
        return
    try:
        assert int(eng.is_complete) == device_props(name)["isComplete"] == PC.expected(name)["isComplete"]
    finally:
        eng.close()


def test_sweep_budget_hands_off_and_back():
    top = PC.cases()["d_two_rings"]
    want = PC.expected("d_two_rings")
    off = E.graph_props(top, device=0, sweep_budget=1, membership=True)
    assert off["info"]["handedOff"] == 1
    PC.assert_props(off, want, "budget 1")
    # Above the case's sweep count.  The count varies a little from run to run (a colour or a
    # hook sweep may carry a label over several arcs), so the bound is reasoned: no phase needs
    # more sweeps than the longest simple path (130 arcs), one confirming sweep and 3 of batch
    # rounding; the phases are the counting sweep, at most 3 trims of 2 steps, the reach, the
    # colour push and the backward reach: 1 + 6 + 3 * 134 = 409.
    used = device_props("d_two_rings")["info"]["sweeps"]
    assert 130 <= used <= 409
    on = E.graph_props(top, device=0, sweep_budget=409, membership=True)
    assert on["info"]["handedOff"] == 0 and on["info"]["sweeps"] <= 409
    PC.assert_props(on, want, "budget above")
    # below it: the pivot's reach alone advances one arc per sweep round a 130-ring
    off = E.graph_props(top, device=0, sweep_budget=100, membership=True)
    assert off["info"]["handedOff"] == 1 and off["info"]["sweeps"] == 100
    PC.assert_props(off, want, "budget 100")


def test_ring_sweeps_are_counted():
    info = device_props("d_ring257")["info"]
    assert info["sweeps"] >= 257 and info["rounds"] >= 2      # a trim and the pivot
    assert info["usCall"] >= info["usDevice"] > 0


def test_decomposition_reaches_colouring_rounds():
    """Trim removes nothing of the chained two-cycles and the pivot takes one
    pair: the other 199 clusters come from colouring rounds."""
    assert device_props("d_two_cycles_chained")["info"]["rounds"] >= 3
    assert device_props("d_chain500")["info"]["rounds"] == 1  # all trimmed


@pytest.mark.parametrize("directed", [False, True])
def test_bad_endpoint_then_valid_call(directed):
    top = PC.cases()["size257_d" if directed else "size257_u"]

    class Bad:
        n, directed = top.n, top.directed
        src, dst = top.src.copy(), top.dst.copy()
    for bad in (top.n, -1):
        Bad.dst[top.m - 1] = bad                              # in the last, partial wave
        with pytest.raises(E.EngineError) as ei:
            E.graph_props(Bad, device=0)
        assert ei.value.code == E.EINVAL
        Bad.dst[top.m - 1] = top.dst[top.m - 1]
        Bad.src[5] = bad
        with pytest.raises(E.EngineError) as ei:
            E.graph_props(Bad, device=0, membership=True)
        assert ei.value.code == E.EINVAL
        Bad.src[5] = top.src[5]
    PC.assert_props(E.graph_props(Bad, device=0, membership=True), PC.expected(top.name), "after EINVAL")


def test_argument_errors_on_the_device():
    lib = E.load_library()
    out, info = E.GraphPropsC(), E.GraphPropsInfoC()
    d = E.GraphDesc(0, 0, 0, None, None, None, None, None)
    assert lib.shd_pe_graph_props(C.byref(d), 0, 0, C.byref(out), None, C.byref(info)) == E.EINVAL
    d = E.GraphDesc(1, 0, 0, None, None, None, None, None)
    assert lib.shd_pe_graph_props(C.byref(d), 0, 0, None, None, None) == E.EINVAL
    assert lib.shd_pe_graph_props(C.byref(d), 1 << 20, 0, C.byref(out), None, None) == E.ENODEV
    assert lib.shd_pe_graph_props(C.byref(d), 0, 0, C.byref(out), None, None) == 0     # info is optional
    assert (out.clusterCount, out.isComplete, out.firstIncomplete) == (1, 0, 0)


def test_shipped_graphml_end_to_end():
    from test_props import shipped_props
    top, host = shipped_props()
    got = E.graph_props(top, device=0, membership=True)
    assert got["info"]["handedOff"] == 0
    PC.assert_props(got, host, "shipped")
    assert got["isComplete"] == 1 and got["clusterCount"] == 1 and got["largestCluster"] == 183
