"""The lane offsets never change a row or a path: the batched kernels with
least-squares offsets (SHDPE_LANE_OFFSET=1, the default) and with the
nearest-hub distances (0) at 8 and 16 lanes, on the small graphs of
tests/plan_cost_cases.py -- a padded last batch, an unreached lane (its batch
falls back to the nearest-hub offsets), fewer hubs than groups, a directed
graph -- and shd_pe_get_paths over a few sources, whose batches (one of them
a one-lane batch at 8 lanes) the path tier composes itself."""
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


def requests(att):
    """9 sources (one full batch of 8 and a one-lane batch; a part of a batch
    of 16), the last attached vertex among them, 3 destinations each."""
    att = np.asarray(att, np.int32)
    srcs = np.append(att[:: max(1, att.shape[0] // 8)][:8], att[-1])
    assert np.unique(srcs).shape[0] == 9
    dsts = att[[1, att.shape[0] // 2, att.shape[0] - 2]]
    return np.repeat(srcs, 3).astype(np.int32), np.tile(dsts, 9).astype(np.int32)


def run(E, top, att, lb, kind, monkeypatch):
    """Paths from a fresh engine (the path tier's own batches), then the table."""
    monkeypatch.setenv("SHDPE_BATCH_LB", str(lb))
    monkeypatch.setenv("SHDPE_LANE_OFFSET", str(kind))
    eng = E.Engine(top, att, force_mode=5, debug_flags=E.DEBUG_ENV)
    assert np.array_equal(eng.attached, att)
    src, dst = requests(att)
    paths = eng.get_paths(src, dst, hops=True)
    info = eng.paths_info()
    eng.compute_all()
    rows = eng.get_rows(0, eng.T)
    st = eng.stats()
    eng.close()
    return {k: rows[k] for k in FIELDS}, st, paths, info


@pytest.mark.parametrize("lb", [8, 16])
@pytest.mark.parametrize("case", list(CASES))
def test_rows_and_paths_do_not_depend_on_lane_offsets(E, expected, monkeypatch, case, lb):
    top, att = CASES[case]
    exp = expected[case]
    ok = (exp["flags"] & 0x03) == 0                # (failed entries carry no values)
    res = {}
    for kind in (1, 0):
        got, st, paths, info = res[kind] = run(E, top, att, lb, kind, monkeypatch)
        ctx = f"{case} lb {lb} lane offsets {kind}"
        assert st["mode"] == 1 and st["batched"] == 1 and st["batchLanes"] == lb, (ctx, st)
        assert np.array_equal(got["flags"] & 0x03, exp["flags"] & 0x03), ctx
        for k in ("lat", "rel"):
            assert np.array_equal(got[k][ok].view(np.int64), exp[k][ok].view(np.int64)), (ctx, k)
        for k in ("hops", "pred"):
            assert np.array_equal(got[k][ok], exp[k][ok]), (ctx, k)
        # tie-free latencies: no row leaves the batched path, none is repaired
        assert st["rowsExact"] == 0 and st["rowsTieRepaired"] == 0, (ctx, st)
        # the batch tier served the path requests from batches of its own (the
        # isolated vertex, which reaches nothing, may be answered before any tier)
        assert info["batch"] >= 8 and info["tie"] == 0 and info["emulated"] == 0, (ctx, info)
    for k in ("batch", "tie", "emulated", "handed_on", "groups"):
        assert res[1][3][k] == res[0][3][k], (case, lb, k, res[1][3], res[0][3])
    for k in FIELDS:
        assert res[1][0][k].tobytes() == res[0][0][k].tobytes(), (case, lb, k)
    assert len(res[1][2]) == len(res[0][2]) == 5
    for a, b in zip(res[1][2], res[0][2]):
        assert a.tobytes() == b.tobytes(), (case, lb, "paths")
    assert (res[1][2][2] == 0).any()               # some path was found
