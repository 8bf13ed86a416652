"""The predecessor filter never changes a row: the split batched kernels with
the on-demand predecessor pass reading only the in-arcs the relax flagged
(the default) and reading every in-arc (SHDPE_PRED_FILTER=0), at 8 and 16
lanes and in the 4-, 6- and 8-wave variants.

Cases: the small graphs of tests/plan_cost_cases.py (ba1200 has a vertex of
degree 114: the wave-scanned heavy entries; `directed` has its own in-arc
lists: the out-arc -> in-arc slot mapping), a graph whose vertices have 17-63
in-arcs (entries of several lane-wide chunks), the quantised ba1200, a
coarsely quantised graph (many tie rows: the deferred tie export, which scans
every in-arc, and the exact kernel) and a multigraph."""
import numpy as np
import pytest

from plan_cost_cases import plan_cost_graphs
from shdpe import generators as G

pytestmark = pytest.mark.gpu

FIELDS = ("lat", "rel", "hops", "flags", "pred")


def _cases():
    # (third: True = continuous latencies, no row leaves the batched path;
    # False = tie rows must occur; None = quantised, ties as they fall)
    c = {name: (top, np.asarray(att, np.int32), True) for name, top, att in plan_cost_graphs()}
    mid = G.random_sparse(300, 36, seed=21)
    c["middeg"] = (mid, G.sample_attached(300, 77, seed=3).astype(np.int32), True)
    c["ba1200q"] = (G.power_law(1200, m=3, seed=4, quantum=0.005),
                    G.sample_attached(1200, 300, seed=2).astype(np.int32), None)
    c["ties"] = (G.random_sparse(500, 5, seed=36, quantum=1.0), np.arange(0, 500, 2, dtype=np.int32), False)
    multi = G.with_parallel_edges(G.random_sparse(400, 5, seed=41, vloss=True), 0.3, seed=7)
    c["multigraph"] = (multi, np.arange(0, 400, 3, dtype=np.int32), True)
    return c


CASES = _cases()


def _degrees(top):
    s, d = np.asarray(top.src), np.asarray(top.dst)
    keep = s != d
    pairs = np.unique(np.stack([np.minimum(s[keep], d[keep]), np.maximum(s[keep], d[keep])]), axis=1)
    return np.bincount(pairs.ravel(), minlength=top.n)


def test_cases_cover_the_scan_paths():
    """The graphs reach the code they are here for (host-side check of the
    generators: heavy entries in ba1200, multi-chunk light entries in middeg)."""
    assert _degrees(CASES["ba1200"][0]).max() >= 64
    deg = _degrees(CASES["middeg"][0])
    assert ((deg >= 17) & (deg <= 63)).sum() >= 250, np.bincount(deg)


@pytest.fixture(scope="module")
def E():
    from shdpe import engine
    engine.load_library()
    return engine


@pytest.fixture(scope="module")
def expected(oracle_mod):
    """The oracle's rows of every case, computed once."""
    return {name: oracle_mod.OracleGraph(top).rows(att, att, threads=8) for name, (top, att, _) in CASES.items()}


def table(E, top, att, lb, wpe, filt, monkeypatch):
    monkeypatch.setenv("SHDPE_BATCH_LB", str(lb))
    monkeypatch.setenv("SHDPE_BATCH_WPE", str(wpe))
    monkeypatch.setenv("SHDPE_PRED_FILTER", "1" if filt else "0")
    eng = E.Engine(top, att, force_mode=5, debug_flags=E.DEBUG_ENV | E.DEBUG_COUNTERS)
    assert np.array_equal(eng.attached, att)
    eng.compute_all()
    rows = eng.get_rows(0, eng.T)
    st = eng.stats()
    eng.close()
    return {k: rows[k] for k in FIELDS}, st


@pytest.mark.parametrize("wpe", [4, 6, 8])
@pytest.mark.parametrize("lb", [8, 16])
@pytest.mark.parametrize("case", list(CASES))
def test_rows_exact_with_and_without_filter(E, expected, monkeypatch, case, lb, wpe):
    top, att, tiefree = CASES[case]
    exp = expected[case]
    ok = (exp["flags"] & 0x03) == 0                # (failed entries carry no values)
    got = {}
    for filt in (True, False):
        rows, st = table(E, top, att, lb, wpe, filt, monkeypatch)
        got[filt] = rows
        ctx = f"{case} lb {lb} wpe {wpe} filter {int(filt)}"
        assert st["mode"] == 1 and st["batched"] == 1 and st["batchLanes"] == lb, (ctx, st)
        assert st["batchWaves"] == wpe and st["batchPostWaves"] == wpe, (ctx, st)
        assert np.array_equal(rows["flags"] & 0x03, exp["flags"] & 0x03), ctx
        for k in ("lat", "rel"):
            assert np.array_equal(rows[k][ok].view(np.int64), exp[k][ok].view(np.int64)), (ctx, k)
        for k in ("hops", "pred"):
            assert np.array_equal(rows[k][ok], exp[k][ok]), (ctx, k)
        assert st["rowsTieRepaired"] == 0, (ctx, st)
        if tiefree:
            assert st["rowsExact"] == 0, (ctx, st)
        elif tiefree is False:
            assert st["rowsExact"] > 0, (ctx, st)       # tie rows: the export and the exact kernel
        claimed, gathered = st["predArcsClaimed"], st["predArcsGathered"]
        print(f"{ctx}: in-arcs claimed {claimed} gathered {gathered}")
        assert claimed > 0, (ctx, st)
        if not filt:
            assert gathered == claimed, (ctx, st)       # no filter: every in-arc of a claimed entry
        else:
            assert gathered <= claimed, (ctx, st)
            if case == "ba1200":
                assert gathered < claimed, (ctx, st)    # a filter that is off cannot pass
    for k in FIELDS:
        assert got[True][k].tobytes() == got[False][k].tobytes(), (case, lb, wpe, k)


@pytest.mark.parametrize("lb", [8, 16])
def test_get_paths_same_under_both_settings(E, monkeypatch, lb):
    """shd_pe_get_paths' pass over the round's distances (the post kernel
    without its row stores) on the directed graph: the same paths."""
    top, att, _ = CASES["directed"]
    rng = np.random.default_rng(5)
    src = rng.choice(att, 200).astype(np.int32)
    dst = rng.choice(att, 200).astype(np.int32)
    out = {}
    for filt in (True, False):
        monkeypatch.setenv("SHDPE_BATCH_LB", str(lb))
        monkeypatch.setenv("SHDPE_PRED_FILTER", "1" if filt else "0")
        eng = E.Engine(top, att, force_mode=5, debug_flags=E.DEBUG_ENV)
        out[filt] = eng.get_paths(src, dst)
        eng.close()
    for a, b in zip(out[True], out[False]):
        assert np.array_equal(a, b)
    offsets, verts, status = out[True]
    assert (np.asarray(status) == 0).sum() > 100          # real paths were compared
