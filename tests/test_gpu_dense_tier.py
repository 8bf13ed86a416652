"""GPU tests of the all-pairs load's parent tier in the dense mode
(shd_pe_table_load_set_parent_tier on a mode-3 engine: launch_dense_rows'
DENSE_PRED stage and k_tree_load_parents over the predecessor pass's vertex-id
parent rows; the tie rows of an undirected graph over the dense tie slots).
Every comparison of sums is exact: against shd_pe_path_load on the explicit
request list and, where stated, numpy over the paths of shd_pe_get_paths or of
the oracle.  The cases are dense_cases.py's, whose premises test_dense_cases.py
pins on the CPU."""
import numpy as np
import pytest

import dense_cases as DC
from test_gpu_path_load import _sum_paths, _usum
from test_gpu_paths import E, _Oracle  # noqa: F401  (E: the fixture)
from test_gpu_table_load import _matrix, _pairs, _reference, _same

pytestmark = pytest.mark.gpu

U64 = np.uint64
SWITCHES = ("SHDPE_TLOAD_TREE", "SHDPE_TLOAD_CORRUPT", "SHDPE_BATCH_GRID", "SHDPE_PATHS_FAST", "SHDPE_TIE_SLOTS",
            "SHDPE_TIE_CORRUPT", "SHDPE_DENSE_BATCH_GB", "SHDPE_PRED_MI", "SHDPE_DENSE_EPOCHS")
TIE_FREE = ["tiny_2", "tiny_17", "edge_129", "edge_257", "dir129", "chain400"]
TIES = ["und97q", "dir257q_holes", "sparse_q"]


@pytest.fixture(autouse=True)
def _clean_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _one_route_each(info, count):
    assert info["tree"] + info["direct"] + info["route"] + info["parents"] + info["tie"] == count, info
    assert 0 <= info["handed_on"] <= info["route"]


def _on(eng):
    eng.set_table_load_parent_tier(True)
    return eng


def _engine(E, name, monkeypatch=None, env=None, att=None, **kw):
    """A mode-3 engine of a dense_cases graph (att: other attached vertices)."""
    top, catt, force = DC.build(name)
    flags = 0
    for k, v in (env or {}).items():
        assert k in SWITCHES, k
        monkeypatch.setenv(k, str(v))
        flags = E.DEBUG_ENV | E.DEBUG_COUNTERS
    eng = E.Engine(top, catt if att is None else np.asarray(att, np.int32), force_mode=force, debug_flags=flags, **kw)
    return eng


def _exact_rows(E, eng):
    return int(np.count_nonzero(np.any(eng.get_rows(0, eng.T)["flags"] & E.F_EXACT, axis=1)))


def _check_counters(E, eng, name, info, count):
    _one_route_each(info, count)
    assert info["tree"] == 0 and info["direct"] == 0
    if name in TIE_FREE:
        assert info["parents"] == count and info["route"] == 0 and info["tie"] == 0
        assert info["parent_claimed"] >= count
    else:                # (und97q, dir257q_holes: every row is a tie row -- all slots, all request route)
        assert info["route"] <= _exact_rows(E, eng)
    if name in ("und97q", "sparse_q", "dense300q"):
        assert info["tie"] >= 1 and info["handed_on"] == 0


# ---- 1. shapes where the kernels can go wrong -----------------------------------

@pytest.mark.parametrize("name", TIE_FREE + TIES)
def test_shapes(E, name):
    eng = _on(_engine(E, name))
    T = eng.T
    w = _matrix(T, T)
    assert np.any(w == 0)
    ref = _reference(eng, 0, T, w)
    assert eng.stats()["mode"] == 3
    got = eng.table_load(weight=w)
    info = eng.table_load_info()
    print(name, info, got["totals"])
    _same(got, ref)
    _check_counters(E, eng, name, info, T)
    if name == "dir257q_holes":
        assert int(got["totals"][3]) > 0
        assert info["tie"] == 0                          # (directed: no dense tie slots)
    if name == "chain400":                               # the ends: one chain of 399 claimed vertices
        assert info["parent_claimed"] >= T * T * 9 // 10
    eng.close()


# ---- 2. chunks ------------------------------------------------------------------

@pytest.mark.parametrize("name", ["edge_129", "dense300q"])
def test_chunks(E, monkeypatch, name):
    """The 64-row floor of ensure_dense: edge_129 in chunks of 64, 64 and 1 rows;
    dense300q's tie rows exported from several chunks."""
    eng = _on(_engine(E, name, monkeypatch, {"SHDPE_DENSE_BATCH_GB": "1e-9"}))
    T = eng.T
    w = _matrix(T, T, seed=21)
    ref = _reference(eng, 0, T, w, paths=False)
    got = eng.table_load(weight=w)
    info = eng.table_load_info()
    print(name, info)
    _same(got, ref)
    _check_counters(E, eng, name, info, T)
    if name == "dense300q":
        assert info["tie"] >= 2
    eng.close()


def test_tie_rows_beyond_the_slots(E, monkeypatch):
    """Two tie slots per chunk: a chunk's further tie rows take the request
    route; no slot at all: every tie row does."""
    counts = {}
    for cap in (2, 0):
        eng = _on(_engine(E, "dense300q", monkeypatch, {"SHDPE_TIE_SLOTS": cap}))
        T = eng.T
        w = _matrix(T, T, seed=22)
        got = eng.table_load(weight=w)
        info = eng.table_load_info()
        _same(got, _reference(eng, 0, T, w, paths=False))
        _one_route_each(info, T)
        assert info["handed_on"] == 0
        counts[cap] = info
        eng.close()
    assert counts[2]["tie"] == 2 and counts[0]["tie"] == 0
    assert counts[0]["route"] == counts[2]["route"] + 2 > 2
    assert counts[0]["parents"] == counts[2]["parents"]


# ---- 3. ranges ------------------------------------------------------------------

def test_ranges(E):
    """Counts around the predecessor tile's height of 32, the ends, no row."""
    eng = _on(_engine(E, "edge_129"))
    T = eng.T
    w = _matrix(T, T, seed=23)
    for start, count in [(0, 31), (1, 32), (5, 33), (0, 1), (T - 1, 1), (0, 0)]:
        got = eng.table_load(start, count, w[start:start + count])
        info = eng.table_load_info()
        if count == 0:
            assert not got["arc"].any() and not got["vertex"].any() and not got["totals"].any()
            assert info["parents"] == info["tie"] == info["route"] == 0
            continue
        _same(got, _reference(eng, start, start + count, w[start:start + count], paths=False))
        assert info["parents"] == count and info["route"] == 0, (start, count, info)
    eng.close()


# ---- 4. weights -----------------------------------------------------------------

def test_weights(E):
    eng = _on(_engine(E, "edge_129"))
    T = eng.T
    none = eng.table_load()
    assert eng.table_load_info()["parents"] == T
    _same(none, eng.table_load(weight=np.ones((T, T), U64)))
    _same(none, _reference(eng, 0, T, None, paths=False))
    # nothing to add: the pairs are still counted
    zero = eng.table_load(weight=np.zeros((T, T), U64))
    assert eng.table_load_info()["parents"] == T
    assert not zero["arc"].any() and not zero["vertex"].any()
    assert int(zero["totals"][0]) == int(none["totals"][0]) == T * T
    assert int(zero["totals"][1]) == int(zero["totals"][2]) == 0
    # sums that wrap
    top_w = np.full((40, T), 2 ** 63 + 12345, U64)
    top_w[:, ::3] = 2 ** 64 - 1
    got = eng.table_load(3, 40, top_w)
    assert eng.table_load_info()["parents"] == 40
    _same(got, _reference(eng, 3, 43, top_w, paths=False))
    assert int(got["totals"][0]) * (2 ** 63) >= 2 ** 64      # (no sum of these fits: every one wrapped)
    # a column slice: a leading dimension past T, garbage behind the rows
    wide = _matrix(T, T, seed=5, ld=T + 5)
    assert wide.shape[1] == T + 5
    _same(eng.table_load(weight=wide), _reference(eng, 0, T, wide, paths=False))
    assert eng.table_load_info()["parents"] == T
    eng.close()


# ---- 5. off by default and switches ---------------------------------------------

def test_off_by_default(E):
    """Without the setter a mode-3 engine serves every source by the request route."""
    eng = _engine(E, "edge_129")
    T = eng.T
    w = _matrix(T, T, seed=2)
    got = eng.table_load(weight=w)
    info = eng.table_load_info()
    assert eng.stats()["mode"] == 3
    _same(got, _reference(eng, 0, T, w, paths=False))
    assert info["parents"] == info["tie"] == info["parent_claimed"] == info["parent_atomics"] == 0
    assert info["route"] == T and info["tree"] == 0 and info["handed_on"] == 0
    eng.close()


def test_setter_switches_the_dense_tier(E):
    eng = _engine(E, "edge_129")
    T = eng.T
    w = _matrix(T, T, seed=2)
    ref = _reference(eng, 0, T, w, paths=False)

    def off():
        _same(eng.table_load(weight=w), ref)
        info = eng.table_load_info()
        assert info["parents"] == info["tie"] == info["parent_claimed"] == 0 and info["route"] == T

    off()
    _on(eng)
    _same(eng.table_load(weight=w), ref)
    info = eng.table_load_info()
    assert info["parents"] == T and info["route"] == 0
    eng.set_table_load_parent_tier(False)
    off()
    eng.close()


def test_paths_fast_switch_turns_it_off(E, monkeypatch):
    eng = _on(_engine(E, "edge_129", monkeypatch, {"SHDPE_PATHS_FAST": 0}))
    got = eng.table_load(0, 5)
    info = eng.table_load_info()
    _same(got, _reference(eng, 0, 5, None, paths=False))
    assert info["parents"] == 0 and info["route"] == 5
    eng.close()


def test_force_mode_3_turns_it_off(E):
    top, att, _ = DC.build("edge_129")
    eng = _on(E.Engine(top, att, force_mode=3))
    got = eng.table_load(0, 5)
    info = eng.table_load_info()
    _same(got, _reference(eng, 0, 5, None, paths=False))
    assert info["parents"] == 0 and info["tie"] == 0 and info["route"] == 5
    eng.close()


# ---- 6. hand-on by injection ----------------------------------------------------

@pytest.mark.parametrize("value", [1, 2, 3])
def test_hand_on(E, monkeypatch, value):
    """The call's first source spoiled: expected total, first parent read, weighted
    vertex count.  The kernel hands it on; nothing of it reached the accumulator
    (the sums are the reference's, and the request route's own share is whole)."""
    eng = _on(_engine(E, "edge_129", monkeypatch, {"SHDPE_TLOAD_CORRUPT": value}))
    T = eng.T
    w = _matrix(T, T, seed=9)
    got = eng.table_load(weight=w)
    info = eng.table_load_info()
    _same(got, _reference(eng, 0, T, w, paths=False))
    _one_route_each(info, T)
    assert info["handed_on"] == 1 and info["route"] == 1 and info["parents"] == T - 1
    assert eng.path_load_info()["entries"] > 0            # (the request route served it)
    # the first source alone: everything comes from the request route
    one = eng.table_load(0, 1, w[:1])
    oinfo = eng.table_load_info()
    _same(one, _reference(eng, 0, 1, w[:1], paths=False))
    assert oinfo["parents"] == 0 and oinfo["handed_on"] == oinfo["route"] == 1 and oinfo["parent_claimed"] == 0
    eng.close()


# ---- 7. no side effects ---------------------------------------------------------

def test_no_side_effects(E):
    eng = _on(_engine(E, "und97q"))
    eng.compute_all()
    T = eng.T
    before, ck, binfo = eng.stats(), eng.row_checksums(0, T), eng.batch_info()
    flags = eng.get_rows(0, T)["flags"].copy()
    w = _matrix(T, T, seed=13)
    got = eng.table_load(weight=w)
    info = eng.table_load_info()
    assert info["tie"] > 0 and info["parents"] + info["tie"] + info["route"] == T
    assert eng.stats() == before
    assert eng.batch_info() == binfo
    assert np.array_equal(eng.row_checksums(0, T), ck)
    assert np.array_equal(eng.get_rows(0, T)["flags"], flags)
    _same(got, _reference(eng, 0, T, w, paths=False))
    eng.close()


# ---- 8. against the oracle ------------------------------------------------------

def test_against_oracle(E, oracle_mod):
    """60 sources of the directed tie-free dense graph, against igraph's paths."""
    top, att, force = DC.build("dir129")
    eng = _on(E.Engine(top, att, force_mode=force))
    orc = _Oracle(oracle_mod, top, eng.attached)
    T = eng.T
    w = _matrix(60, T, seed=8)
    src, dst = _pairs(att, 0, 60)
    paths = [orc.path(s, t) for s, t in zip(src, dst)]
    assert all(p is not None for p in paths)
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
    arc, vertex = _sum_paths(eng, offsets, np.concatenate(paths), w.reshape(-1))
    got = eng.table_load(0, 60, w)
    info = eng.table_load_info()
    assert np.array_equal(got["arc"], arc) and np.array_equal(got["vertex"], vertex)
    _same(got, _reference(eng, 0, 60, w, paths=False))
    assert info["parents"] == 60 and info["route"] == 0
    eng.close()


# ---- 9. shards ------------------------------------------------------------------

def test_three_local_shards(E):
    eng = _on(_engine(E, "edge_257"))
    T = eng.T
    w = _matrix(T, T, seed=12)
    ref = _reference(eng, 0, T, w, paths=False)
    whole = eng.table_load(weight=w)
    assert eng.table_load_info()["parents"] == T
    eng.close()
    _same(whole, ref)
    eng = _on(_engine(E, "edge_257", devices=[0, 0, 0]))
    bounds = eng.shard_bounds()
    assert len(bounds) == 4 and 0 < bounds[1] < bounds[2] < T
    lo, hi = int(bounds[1]) - 20, int(bounds[2]) + 30          # spans all three
    assert 0 <= lo and hi <= T
    got = eng.table_load(weight=w)
    info = eng.table_load_info()
    part = eng.table_load(lo, hi - lo, w[lo:hi])
    pinfo = eng.table_load_info()
    _same(part, _reference(eng, lo, hi, w[lo:hi], paths=False))
    eng.close()
    _same(got, ref)
    for key in ("arc", "vertex", "totals"):
        assert np.array_equal(got[key], whole[key]), key
    assert info["parents"] == T and info["route"] == 0
    assert pinfo["parents"] == hi - lo and pinfo["route"] == 0
    _one_route_each(info, T)
    _one_route_each(pinfo, hi - lo)


# ---- 10. one source -------------------------------------------------------------

def test_one_attached_vertex(E):
    eng = _on(_engine(E, "edge_129", att=[17]))
    w = np.array([[5]], U64)
    got = eng.table_load(weight=w)
    info = eng.table_load_info()
    assert eng.stats()["mode"] == 3
    _same(got, _reference(eng, 0, 1, w))
    assert int(got["vertex"][17]) == 5 and _usum(got["vertex"]) == 5 and not got["arc"].any()
    assert info["parents"] == 1 and info["parent_claimed"] == 1 and info["route"] == 0
    eng.close()
