"""GPU parity of the dense min-plus path (mode 3: pe_dense.hip, k_exact_dense
and the dense branches of the engine's relax / exact stages) at the edges the
other dense tests do not reach: tile and chunk remainders of k_minplus,
directed graphs, deep rows, low-degree vertices, the debug switches, partial
attachment with unreachable targets and missing self-loops.  The cases come
from dense_cases.py; test_dense_cases.py checks their premises on the CPU.

Every comparison is bit-exact against the oracle, flags & 0x07 on every entry
included."""
import numpy as np
import pytest

import dense_cases as DC
from test_gpu_parity import _assert_rows_equal
from test_gpu_paths import _Oracle, _check_against_oracle, _requests

pytestmark = pytest.mark.gpu

FIELDS = ("lat", "rel", "hops", "pred", "flags")


@pytest.fixture(scope="module")
def E():
    from shdpe import engine
    engine.load_library()
    return engine


_CASES, _EXPECTED, _TIES, _DEFAULT = {}, {}, {}, {}


def _case(name):
    if name not in _CASES:
        _CASES[name] = DC.build(name)
    return _CASES[name]


def _expected(oracle_mod, name):
    """The oracle's whole table of a case (attached x attached), computed once
    and read-only."""
    if name not in _EXPECTED:
        top, att, _ = _case(name)
        og = oracle_mod.OracleGraph(top)
        rows = og.rows(att, att, threads=8)
        for a in rows.values():
            a.setflags(write=False)
        _EXPECTED[name] = (og, rows)
    return _EXPECTED[name]


def _n_tie_rows(oracle_mod, name):
    if name not in _TIES:
        top, att, _ = _case(name)
        _TIES[name] = len(DC.tie_rows(_expected(oracle_mod, name)[0], top, att))
    return _TIES[name]


def _assert_exact(got, exp, ctx):
    """_assert_rows_equal, and the flag bits it masks out (F_ZEROLAT)."""
    _assert_rows_equal(got, exp, ctx)
    assert np.array_equal(got["flags"] & 0x07, exp["flags"] & 0x07), ctx


def _rows_at(exp, idx):
    return {k: v[idx] for k, v in exp.items()}


def _engine(E, name, debug_flags=0):
    top, att, force = _case(name)
    eng = E.Engine(top, att, force_mode=force, debug_flags=debug_flags)
    assert np.array_equal(eng.attached, att)
    return eng


def _check_sources(E, oracle_mod, name, sources, debug_flags=0):
    """A fresh engine computing `sources` alone; those rows against the oracle."""
    _, att, _ = _case(name)
    _, exp = _expected(oracle_mod, name)
    eng = _engine(E, name, debug_flags)
    eng.compute_rows(np.asarray(sources, np.int32))
    st = eng.stats()
    for s in sources:
        i = int(np.searchsorted(att, s))
        _assert_exact(eng.get_row(int(s)), _rows_at(exp, i), f"{name} row {s}")
    eng.close()
    assert st["mode"] == 3 and st["rowsTieRepaired"] == 0, st
    assert st["rowsComputed"] == len(sources), st
    return st


def _whole_table(E, oracle_mod, name, debug_flags=0):
    """compute_all on a fresh engine: (table, stats), the table checked
    against the oracle."""
    _, exp = _expected(oracle_mod, name)
    eng = _engine(E, name, debug_flags)
    eng.compute_all()
    got = eng.get_rows(0, eng.T)
    st = eng.stats()
    eng.close()
    _assert_exact(got, exp, name)
    assert st["mode"] == 3 and st["rowsTieRepaired"] == 0, st
    assert st["rowsComputed"] == got["lat"].shape[0], st
    return got, st


def _default_table(E, oracle_mod, name):
    if name not in _DEFAULT:
        got, st = _whole_table(E, oracle_mod, name)
        for a in got.values():
            a.setflags(write=False)
        _DEFAULT[name] = (got, st)
    return _DEFAULT[name]


@pytest.mark.parametrize("name", DC.SIZES)
def test_dense_sizes(E, oracle_mod, name):
    """Every attached row of every size / graph kind against the oracle; the
    tie rows are the ones the oracle's distances predict (two tight in-arcs of
    equal minimal distance) and take the form their graph calls for: early
    stop on undirected graphs, the full k_exact_dense emulation on directed
    ones."""
    _, st = _default_table(E, oracle_mod, name)
    ties = _n_tie_rows(oracle_mod, name)
    print(name, "tie rows", ties, {k: st[k] for k in ("rowsExact", "rowsTieEarly", "denseSweeps")})
    assert st["launchesDense"] == 1, st
    if name in DC.TIE_UNDIRECTED:
        assert st["rowsTieEarly"] == st["rowsExact"] > 0, st
    elif name in DC.TIE_DIRECTED:
        assert st["rowsExact"] > 0 and st["rowsTieEarly"] == 0, st
    elif name in DC.TIE_FREE:
        assert st["rowsExact"] == 0, st
    assert st["rowsExact"] == ties, st


@pytest.mark.parametrize("k", DC.ROWS_K)
def test_dense_row_tile_edges(E, oracle_mod, k):
    """nRows on either side of the PRED (32) and SWEEP (96) tile heights."""
    _, att, _ = _case("edge_129")
    _check_sources(E, oracle_mod, "edge_129", att[:k].tolist())


def test_dense_deep_chain(E, oracle_mod):
    """A 400-vertex path graph forced dense.  From source 0 the in-place sweeps
    advance one hop each: 399 sweeps seen on the MI355X, so the chunk epochs
    (uint8, off from sweep 249) hand over to full sweeps mid-row and the last
    149 sweeps run without them; k_dense_write folds chains of up to 399
    hops."""
    st = _check_sources(E, oracle_mod, "chain400", [0])
    print("chain400 source 0: denseSweeps", st["denseSweeps"])
    # (rowsExact: a row the sweeps left short of its fixpoint has entries
    # without a tight predecessor and would be handed to the emulation)
    assert st["denseSweeps"] > 250 and st["rowsExact"] == 0, st
    st = _check_sources(E, oracle_mod, "chain400", [399, 200, 133, 7])
    assert st["rowsExact"] == 0, st


SWITCHES = {
    "pred_mi3": ("SHDPE_PRED_MI", "3"),
    "pred_mi4": ("SHDPE_PRED_MI", "4"),
    "pred_mi6": ("SHDPE_PRED_MI", "6"),
    "epochs0": ("SHDPE_DENSE_EPOCHS", "0"),
    "batch64": ("SHDPE_DENSE_BATCH_GB", "1e-9"),     # the 64-row floor of ensure_dense
}


@pytest.mark.parametrize("name,switch",
                         [(n, s) for n in ("und97q", "dir129q", "sparse_q", "dense300q") for s in SWITCHES]
                         + [("chain400", "epochs0")])
def test_dense_switches(E, oracle_mod, monkeypatch, name, switch):
    """Each dense switch gives the default engine's table byte for byte (and
    that one is the oracle's); the deep chain once with full sweeps from the
    start."""
    top, att, _ = _case(name)
    if name == "chain400":
        monkeypatch.setenv(*SWITCHES[switch])
        st = _check_sources(E, oracle_mod, name, [0, 200], debug_flags=E.DEBUG_ENV)
        assert st["denseSweeps"] > 250 and st["rowsExact"] == 0, st
        return
    ref, ref_st = _default_table(E, oracle_mod, name)
    var, val = SWITCHES[switch]
    monkeypatch.setenv(var, val)
    got, st = _whole_table(E, oracle_mod, name, debug_flags=E.DEBUG_ENV)
    for k in FIELDS:
        assert got[k].tobytes() == ref[k].tobytes(), (name, switch, k)
    assert st["rowsExact"] == ref_st["rowsExact"] > 0, st
    T = att.shape[0]
    if switch == "batch64":
        assert st["launchesDense"] == (T + 63) // 64, st
        if T == 300:
            assert st["launchesDense"] == 5, st
        if T > 64 or top.directed:
            # several dense chunks: D / P no longer hold the rows, so the
            # undirected tie rows take the general form as well
            assert st["rowsTieEarly"] == 0 < st["rowsExact"], st
        else:
            assert st["rowsTieEarly"] == st["rowsExact"], st
    else:
        assert st["launchesDense"] == 1, st
        assert st["rowsTieEarly"] == ref_st["rowsTieEarly"], st


@pytest.mark.parametrize("name", ["dir129q", "dir257q_holes"])
def test_dense_paths_directed(E, oracle_mod, name):
    """shd_pe_get_paths on directed dense graphs: paths and per-hop attributes
    against the oracle's raw Dijkstra, unreachable targets EUNREACHABLE."""
    top, att, force = _case(name)
    eng = _engine(E, name)
    orc = _Oracle(oracle_mod, top, eng.attached)
    src, dst = _requests(att)
    # (latencies are multiples of 25: every fold order gives the same sum)
    _, _, status, _, _ = _check_against_oracle(E, eng, orc, src, dst, True)
    st = eng.stats()
    eng.close()
    assert st["mode"] == 3, st
    if name == "dir257q_holes":
        assert np.any(status == E.EUNREACHABLE) and np.any(status == 0)
    else:
        assert np.all(status == 0)
