"""The batch schedule never changes a row: the batched kernels under batch
orders 0, 1 and 2 (SHDPE_BATCH_ORDER) at 8 and 16 lanes, on the small graphs
of tests/native/plan_cost.cpp -- fewer hubs than groups, one hub, directed, an
attached vertex no hub reaches, padded last batches."""
import numpy as np
import pytest

from plan_cost_cases import plan_cost_graphs

pytestmark = pytest.mark.gpu

CASES = {name: (top, att) for name, top, att in plan_cost_graphs()}
FIELDS = ("lat", "rel", "hops", "flags", "pred")


@pytest.fixture(scope="module")
def E():
    from shdpe import engine
    engine.load_library()
    return engine


@pytest.fixture(scope="module")
def expected(oracle_mod):
    """The oracle's rows of every case, computed once."""
    exp = {}
    for name, (top, att) in CASES.items():
        exp[name] = oracle_mod.OracleGraph(top).rows(np.asarray(att, np.int32), np.asarray(att, np.int32), threads=8)
    return exp


def table(E, top, att, lb, order, monkeypatch):
    monkeypatch.setenv("SHDPE_BATCH_LB", str(lb))
    monkeypatch.setenv("SHDPE_BATCH_ORDER", str(order))
    eng = E.Engine(top, att, force_mode=5, debug_flags=E.DEBUG_ENV)
    assert np.array_equal(eng.attached, att)
    eng.compute_all()
    rows = eng.get_rows(0, eng.T)
    st = eng.stats()
    eng.close()
    return {k: rows[k] for k in FIELDS}, st


@pytest.mark.parametrize("lb", [8, 16])
@pytest.mark.parametrize("case", list(CASES))
def test_rows_exact_under_every_batch_order(E, expected, monkeypatch, case, lb):
    top, att = CASES[case]
    exp = expected[case]
    ok = (exp["flags"] & 0x03) == 0                # (failed entries carry no values)
    first = None
    for order in (0, 1, 2):
        got, st = table(E, top, att, lb, order, monkeypatch)
        ctx = f"{case} lb {lb} order {order}"
        assert st["mode"] == 1 and st["batched"] == 1 and st["batchLanes"] == lb, (ctx, st)
        assert np.array_equal(got["flags"] & 0x03, exp["flags"] & 0x03), ctx
        for k in ("lat", "rel"):
            assert np.array_equal(got[k][ok].view(np.int64), exp[k][ok].view(np.int64)), (ctx, k)
        for k in ("hops", "pred"):
            assert np.array_equal(got[k][ok], exp[k][ok]), (ctx, k)
        # tie-free latencies: no row leaves the batched path, none is repaired
        assert st["rowsExact"] == 0 and st["rowsTieRepaired"] == 0, (ctx, st)
        if first is None:
            first = got
        for k in got:
            assert got[k].tobytes() == first[k].tobytes(), (ctx, k, "differs from order 0")
