"""GPU tests of the all-pairs load of a range of source rows
(shd_pe_table_load): the sums against shd_pe_path_load on the explicit request
list and against numpy over the paths shd_pe_get_paths returns, exactly; in
every mode, on the shapes where the tree kernel can go wrong (deep trees, one
hub, every lane width, several rounds, reused scratch slots, sub-ranges), with
every kind of weight, with the hand-on injected, across shards, with every
error of the definition, and without side effects."""
import ctypes as C
import os

import numpy as np
import pytest

from shdpe import generators as G
from shdpe.graph import Topology
from test_gpu_parity import _chain
from test_gpu_path_load import COMPLETE, _engine, _sum_paths, _usum, _weights
from test_gpu_paths import CASES, E, _Oracle  # noqa: F401  (E: the fixture)

pytestmark = pytest.mark.gpu

U64 = np.uint64
SWITCHES = ("SHDPE_TLOAD_TREE", "SHDPE_TLOAD_CORRUPT", "SHDPE_BATCH_LB", "SHDPE_BATCH_GRID", "SHDPE_BATCH_ROUND",
            "SHDPE_POST_SPLIT", "SHDPE_PATHS_FAST")


@pytest.fixture(autouse=True)
def _clean_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _pairs(att, lo, hi):
    """The request list table_load(lo, hi - lo) stands for, source-major."""
    att = np.asarray(att, np.int32)
    return np.repeat(att[lo:hi], att.shape[0]), np.tile(att, hi - lo)


def _reference(eng, lo, hi, w, paths=True):
    """Both references of rows [lo, hi) with the weight matrix w (None: ones):
    path_load on the explicit list, and numpy over get_paths' paths."""
    src, dst = _pairs(eng.attached, lo, hi)
    wl = np.ones(src.shape[0], U64) if w is None else np.ascontiguousarray(w[:, :eng.T]).reshape(-1)
    ref = eng.path_load(src, dst, wl)
    if paths:
        offsets, verts, status = eng.get_paths(src, dst)
        assert np.array_equal(status, ref["status"])
        arc, vertex = _sum_paths(eng, offsets, verts, wl)
        assert np.array_equal(arc, ref["arc"]) and np.array_equal(vertex, ref["vertex"])
    return ref


def _same(got, ref):
    assert "status" not in got
    assert np.array_equal(got["arc"], ref["arc"])
    assert np.array_equal(got["vertex"], ref["vertex"])
    assert np.array_equal(got["totals"], ref["totals"])
    assert int(got["totals"][1]) == _usum(got["vertex"])
    assert int(got["totals"][2]) == _usum(got["arc"])


def _one_route_each(info, count):
    assert info["tree"] + info["direct"] + info["route"] == count, info
    assert 0 <= info["handed_on"] <= info["route"]


def _matrix(count, T, seed=7, ld=None):
    w = _weights(count * T, seed=seed).reshape(count, T)
    if ld is None:
        return w
    wide = np.full((count, ld), 0xDEADBEEFCAFEF00D, U64)     # garbage in the padding
    wide[:, :T] = w
    return wide[:, :]


# ---- 1. every mode --------------------------------------------------------------

MODES = list(CASES) + [COMPLETE]


def _directed_with_unreachable(E):
    """directed_batched must hold an unreachable pair.  The generator's directed
    graphs are strongly connected whatever the seed, so the case's graph gets one
    more vertex with an out-arc only, attached: no other source reaches it."""
    base = CASES["directed_batched"][0]()
    n = base.n
    top = Topology(n=n + 1, directed=True, src=np.concatenate([base.src, [n]]), dst=np.concatenate([base.dst, [0]]),
                   latency=np.concatenate([base.latency, [3.0]]), loss=np.concatenate([base.loss, [0.0]]))
    att = np.concatenate([np.arange(0, n, 3), [n]]).astype(np.int32)
    eng = E.Engine(top, att, force_mode=CASES["directed_batched"][2])
    src, dst = _pairs(att, 0, att.shape[0])
    assert np.any(eng.get_paths(src, dst)[2] == E.EUNREACHABLE)
    return eng, att


@pytest.mark.parametrize("name", MODES)
def test_every_mode(E, name):
    eng, att = _directed_with_unreachable(E) if name == "directed_batched" else _engine(E, name)
    T = eng.T
    w = _matrix(T, T)
    assert np.any(w == 0)
    ref = _reference(eng, 0, T, w)
    got = eng.table_load(weight=w)
    info = eng.table_load_info()
    print(name, info, got["totals"])
    _same(got, ref)
    _one_route_each(info, T)
    # ... and the table's flags and hops alone give the totals
    if name != COMPLETE:
        rows = eng.get_rows(0, T)
        ok = (rows["flags"] & E.F_FAILED) == 0
        np.fill_diagonal(ok, True)
        hops = rows["hops"].astype(U64)
        np.fill_diagonal(hops, 0)
        assert int(got["totals"][0]) == np.count_nonzero(ok)
        assert int(got["totals"][3]) == T * T - np.count_nonzero(ok)
        assert int(got["totals"][2]) == _usum(w * hops * ok.astype(U64))
        assert int(got["totals"][1]) == _usum(w * (hops + U64(1)) * ok.astype(U64))
        exact_rows = np.count_nonzero(np.any(rows["flags"] & E.F_EXACT, axis=1))
    if name in ("tiefree_batched", "directed_batched"):
        assert info["tree"] == T and info["route"] == 0
    elif name in ("quantized_batched", "powerlaw_batched"):
        assert exact_rows > 0
        assert info["tree"] > 0 and info["handed_on"] == 0 and info["route"] <= exact_rows
    elif name == COMPLETE:
        assert info["direct"] == T
    else:
        assert info["route"] == T
    if name == "directed_batched":
        assert int(got["totals"][3]) > 0
    if info["tree"]:
        assert info["claimed"] > 0 and info["rounds"] >= 1
    eng.close()


def test_against_oracle(E, oracle_mod):
    """60 sources of the tie-free graph on the batched kernels, against igraph's paths."""
    top = CASES["tiefree"][0]()
    att = np.arange(0, top.n, 3, dtype=np.int32)
    eng = E.Engine(top, att, force_mode=5)
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
    assert info["tree"] == 60 and info["route"] == 0
    eng.close()


# ---- 2. shapes where the new kernels can go wrong -------------------------------

def _env_engine(E, monkeypatch, top, att, env, **kw):
    for k, v in env.items():
        assert k in SWITCHES, k
        monkeypatch.setenv(k, str(v))
    return E.Engine(top, att, force_mode=5, debug_flags=E.DEBUG_ENV | E.DEBUG_COUNTERS, **kw)


def _chain_sums(n, att, lo, hi, w):
    """The loads of a path graph in closed form: the path s -> t is the interval."""
    src, dst = _pairs(att, lo, hi)
    wl = w.reshape(-1)
    a, b = np.minimum(src, dst).astype(np.int64), np.maximum(src, dst).astype(np.int64)
    diff = np.zeros(n + 1, U64)
    np.add.at(diff, a, wl)
    np.subtract.at(diff, b + 1, wl)
    vertex = np.cumsum(diff[:-1], dtype=U64)
    up, down = np.zeros(n + 1, U64), np.zeros(n + 1, U64)    # arcs v -> v + 1 and v + 1 -> v
    fwd = src < dst
    np.add.at(up, a[fwd], wl[fwd])
    np.subtract.at(up, b[fwd], wl[fwd])
    np.add.at(down, a[~fwd], wl[~fwd])
    np.subtract.at(down, b[~fwd], wl[~fwd])
    return vertex, np.cumsum(up[:-1], dtype=U64), np.cumsum(down[:-1], dtype=U64)


@pytest.mark.parametrize("n", [300, 4200])
def test_deep_tree(E, n):
    """A path graph: the tree of a source is as high as the graph is long (past
    LMAX at n = 4,200), and the leaves-first sum has one ready vertex at a time."""
    top = _chain(n, seed=n)
    first = [0, n - 1, n // 2]
    att = np.array(first + [v for v in range(n) if v not in first], np.int32)
    eng = E.Engine(top, att, force_mode=5)
    ranges = [(0, 3)] + ([(0, n)] if n == 300 else [])
    for lo, hi in ranges:
        w = _matrix(hi - lo, n, seed=n + hi)
        got = eng.table_load(lo, hi - lo, w)
        info = eng.table_load_info()
        print(n, (lo, hi), info)
        _same(got, _reference(eng, lo, hi, w, paths=n == 300))
        vertex, up, down = _chain_sums(n, att, lo, hi, w)
        assert np.array_equal(got["vertex"], vertex)
        for v in (0, n // 3, n - 2):
            assert int(got["arc"][eng.find_arc(v, v + 1)]) == int(up[v])
            assert int(got["arc"][eng.find_arc(v + 1, v)]) == int(down[v])
        assert info["tree"] == hi - lo and info["route"] == 0
        assert info["claimed"] >= (hi - lo) * n * 9 // 10     # (a weight-0 leaf end is not claimed)
    eng.close()


def test_hub(E):
    """A star of 400 leaves and a slow ring over them: every leaf-to-leaf path runs
    through the centre, whose sum and pending count take 399 adds per lane."""
    L = 400
    leaves = np.arange(1, L + 1)
    src = np.concatenate([np.zeros(L, np.int64), leaves, np.arange(L + 1)])
    dst = np.concatenate([leaves, np.roll(leaves, -1), np.arange(L + 1)])
    rng = np.random.default_rng(5)
    lat = np.concatenate([rng.uniform(1.0, 2.0, L), rng.uniform(50.0, 60.0, L), np.ones(L + 1)])
    top = Topology(L + 1, False, src, dst, lat, np.zeros(src.shape[0]))
    att = np.arange(L + 1, dtype=np.int32)
    eng = E.Engine(top, att, force_mode=5)
    assert 2 * L > eng.sparse_info()["heavyDeg"]
    w = _matrix(L + 1, L + 1, seed=3)
    ref = _reference(eng, 0, L + 1, w)
    got = eng.table_load(weight=w)
    info = eng.table_load_info()
    _same(got, ref)
    # every leaf-to-leaf pair crosses the centre
    through = _usum(w) - _usum(np.diag(w)[1:])
    assert int(got["vertex"][0]) == through
    assert info["tree"] == L + 1 and info["route"] == 0
    eng.close()


@pytest.mark.parametrize("lb", [4, 8, 16, 32])
def test_lane_widths(E, monkeypatch, lb):
    top = G.random_sparse(500, 5, seed=21)
    att = np.arange(0, 37 * 13, 13, dtype=np.int32)
    assert att.shape[0] == 37
    eng = _env_engine(E, monkeypatch, top, att, {"SHDPE_BATCH_LB": lb})
    w = _matrix(37, 37, seed=lb)
    got = eng.table_load(weight=w)
    info = eng.table_load_info()
    _same(got, _reference(eng, 0, 37, w))
    assert info["tree"] == 37 and info["route"] == 0
    assert 0 < info["atomics"] <= 2 * info["claimed"]
    eng.close()


@pytest.mark.parametrize("grid,rnd,split", [(1, 1, 0), (2, 3, 0), (1, 1, 1), (2, 3, 1)])
def test_rounds_and_post_forms(E, monkeypatch, grid, rnd, split):
    """Several rounds of the pass, and (2, 3) three batches on two scratch slots:
    a workgroup's slot is reused for its second batch."""
    top = G.random_sparse(500, 5, seed=21)
    att = np.arange(0, 500, 5, dtype=np.int32)
    eng = _env_engine(E, monkeypatch, top, att, {"SHDPE_BATCH_LB": 8, "SHDPE_BATCH_GRID": grid,
                                                 "SHDPE_BATCH_ROUND": rnd, "SHDPE_POST_SPLIT": split})
    w = _matrix(100, 100, seed=grid + rnd)
    got = eng.table_load(weight=w)
    info = eng.table_load_info()
    _same(got, _reference(eng, 0, 100, w))
    assert info["tree"] == 100 and info["route"] == 0
    assert info["rounds"] == -(-13 // rnd) > 1                # 100 sources in 13 batches of 8
    eng.close()


def test_sub_ranges(E):
    eng, att = _engine(E, "tiefree_batched")
    T = eng.T
    w = _matrix(T, T, seed=4)
    whole = eng.table_load(weight=w)
    got = eng.table_load(5, 23, w[5:28])
    assert eng.table_load_info()["tree"] == 23
    _same(got, _reference(eng, 5, 28, w[5:28]))
    one = eng.table_load(T - 1, 1, w[T - 1:])
    assert eng.table_load_info()["tree"] == 1
    _same(one, _reference(eng, T - 1, T, w[T - 1:]))
    none = eng.table_load(9, 0)
    assert not none["arc"].any() and not none["vertex"].any() and not none["totals"].any()
    info = eng.table_load_info()
    assert info["tree"] == info["direct"] == info["route"] == 0
    k = 101
    a, b = eng.table_load(0, k, w[:k]), eng.table_load(k, T - k, w[k:])
    for key in ("arc", "vertex", "totals"):
        assert np.array_equal(a[key] + b[key], whole[key]), key
    eng.close()


# ---- 3. weights -----------------------------------------------------------------

def test_weights(E):
    eng, att = _engine(E, "tiefree_batched")
    T = eng.T
    ones = eng.table_load(weight=np.ones((T, T), U64))
    none = eng.table_load()
    _same(none, ones)
    _same(none, _reference(eng, 0, T, None))
    # a leading dimension past T, garbage behind the rows
    wide = _matrix(T, T, seed=5, ld=T + 5)
    got = eng.table_load(weight=wide)
    _same(got, _reference(eng, 0, T, wide))
    # sums that wrap
    top_w = np.full((40, T), 2 ** 64 - 1, U64)
    got = eng.table_load(3, 40, top_w)
    _same(got, _reference(eng, 3, 43, top_w))
    assert int(got["vertex"].max()) > 2 ** 63                # (-k mod 2^64)
    # an all-zero row among the others, and nothing but zeros
    w = _matrix(T, T, seed=6)
    w[17] = 0
    got = eng.table_load(weight=w)
    _same(got, _reference(eng, 0, T, w))
    assert eng.table_load_info()["tree"] == T
    zero = eng.table_load(weight=np.zeros((T, T), U64))
    assert not zero["arc"].any() and not zero["vertex"].any()
    assert zero["totals"].tolist() == [int(ones["totals"][0]), 0, 0, int(ones["totals"][3])]
    assert int(ones["totals"][0]) + int(ones["totals"][3]) == T * T
    eng.close()


# ---- 4. hand-on by injection ----------------------------------------------------

@pytest.mark.parametrize("switch,value", [("SHDPE_TLOAD_CORRUPT", 1), ("SHDPE_TLOAD_CORRUPT", 2),
                                          ("SHDPE_TLOAD_TREE", 0)])
def test_hand_on(E, monkeypatch, switch, value):
    make, _, force, _ = CASES["tiefree_batched"]
    top = make()
    att = np.arange(0, top.n, 3, dtype=np.int32)
    eng = _env_engine(E, monkeypatch, top, att, {switch: value})
    T = eng.T
    w = _matrix(T, T, seed=9)
    got = eng.table_load(weight=w)
    info = eng.table_load_info()
    pinfo, linfo = eng.paths_info(), eng.path_load_info()
    _same(got, _reference(eng, 0, T, w))
    _one_route_each(info, T)
    if switch == "SHDPE_TLOAD_TREE":
        assert info["tree"] == 0 and info["route"] == T and info["handed_on"] == 0
    else:
        assert info["handed_on"] >= 1 and info["route"] == info["handed_on"]
        assert info["tree"] == T - info["handed_on"]
        assert info["handed_on"] == 1                         # the first source alone
    # the request route's info words describe its part of the call
    assert linfo["entries"] > 0 and pinfo["batch"] + pinfo["tie"] + pinfo["emulated"] + pinfo["rows"] > 0
    eng.close()


def test_request_route_info_is_zero_without_it(E):
    eng, att = _engine(E, "tiefree_batched")
    eng.path_load(att[:4], att[4:8])
    assert eng.path_load_info()["entries"] > 0
    eng.table_load()
    assert eng.table_load_info()["route"] == 0
    assert eng.path_load_info() == {"entries": 0, "atomics": 0}
    assert not any(eng.paths_info().values())
    eng.close()


# ---- 5. vertex loss, parallel edges, latFold ------------------------------------

@pytest.mark.parametrize("kind", ["vloss", "parallel", "latfold"])
def test_graph_kinds(E, kind):
    if kind == "vloss":
        top = G.random_sparse(600, 5, seed=35, vloss=True)
    elif kind == "parallel":
        top = G.with_parallel_edges(G.random_sparse(600, 5, seed=36), 0.3, seed=5, consistent=True)
    else:
        top = G.with_slower_newest_edges(G.random_sparse(300, 4, seed=2), 0.4, seed=4)
    att = np.arange(0, top.n, 3, dtype=np.int32)
    eng = E.Engine(top, att, force_mode=5)
    T = eng.T
    w = _matrix(T, T, seed=11)
    got = eng.table_load(weight=w)
    info = eng.table_load_info()
    print(kind, info)
    _same(got, _reference(eng, 0, T, w))
    _one_route_each(info, T)
    if kind == "latfold":
        assert info["route"] == T
    else:
        assert info["tree"] > 0 and info["handed_on"] == 0
    if kind == "parallel":
        assert eng.arcs()[0].shape[0] < 2 * top.m             # arcs are merged groups
    eng.close()


# ---- 6. shards and ownership ----------------------------------------------------

def test_two_local_shards(E):
    eng, att = _engine(E, "quantized_batched")
    T = eng.T
    w = _matrix(T, T, seed=12)
    ref = eng.table_load(weight=w)
    eng.close()
    eng, _ = _engine(E, "quantized_batched", devices=[0, 0])
    bounds = eng.shard_bounds()
    assert len(bounds) == 3 and 0 < bounds[1] < T
    lo, hi = int(bounds[1]) - 20, int(bounds[1]) + 30
    got = eng.table_load(weight=w)
    info = eng.table_load_info()
    part = eng.table_load(lo, hi - lo, w[lo:hi])
    _same(part, _reference(eng, lo, hi, w[lo:hi], paths=False))
    eng.close()
    _same(got, ref)
    _one_route_each(info, T)
    assert info["tree"] > 0


def _raw_call(E, eng, start, count, weight, ld, fill=0x77):
    """shd_pe_table_load on pattern-filled outputs -> (rc, outputs untouched?)."""
    n_arcs = eng.arcs()[0].shape[0]
    arc, vert, tot = (np.full(k, fill, U64) for k in (n_arcs, eng.top.n, 4))
    o = E.LoadOutC(arc.ctypes.data, vert.ctypes.data, None, tot.ctypes.data)
    i = E.TableLoadInC(start, count, None if weight is None else weight.ctypes.data, ld)
    rc = eng._lib.shd_pe_table_load(eng.h, C.byref(i), C.byref(o))
    return rc, all(np.all(a == fill) for a in (arc, vert, tot))


def test_not_owned(E):
    top = CASES["tiefree_batched"][0]()
    att = np.arange(0, top.n, 3, dtype=np.int32)
    eng = E.Engine(top, att, force_mode=5, shard_count=2, shard_index=0)
    T = eng.T
    bounds = eng.shard_bounds()
    own = int(bounds[1])
    assert 0 < own < T
    assert _raw_call(E, eng, 0, T, None, 0) == (E.ENOTOWNED, True)
    assert _raw_call(E, eng, own - 3, 4, None, 0) == (E.ENOTOWNED, True)
    rc, untouched = _raw_call(E, eng, 0, own, None, 0)
    assert rc == 0 and not untouched
    got = eng.table_load(0, own)
    eng.close()
    eng = E.Engine(top, att, force_mode=5)
    _same(got, _reference(eng, 0, own, None, paths=False))
    eng.close()


# ---- 7. errors ------------------------------------------------------------------

def test_errors(E):
    eng, att = _engine(E, "tiefree_batched")
    T = eng.T
    w = np.ones((T, T + 2), U64)
    for start, count, weight, ld in [(-1, 2, None, 0), (0, -1, None, 0), (0, T + 1, None, 0), (T, 1, None, 0),
                                     (5, T - 4, None, 0), (2 ** 31 - 1, 2, None, 0), (0, 3, w, T - 1), (0, 3, w, 0)]:
        assert _raw_call(E, eng, start, count, weight, ld) == (E.EINVAL, True), (start, count, ld)
    i = E.TableLoadInC(0, 1, None, 0)
    assert eng._lib.shd_pe_table_load(eng.h, C.byref(i), None) == E.EINVAL
    assert eng._lib.shd_pe_table_load(eng.h, None, None) == E.EINVAL
    rc, untouched = _raw_call(E, eng, T, 0, None, 0)          # the empty range at the end: zeros
    assert rc == 0 and not untouched
    with pytest.raises(E.EngineError) as err:
        eng.table_load(3, T)
    assert err.value.code == E.EINVAL
    eng.close()


# ---- 8. no side effects ---------------------------------------------------------

def test_no_side_effects(E):
    eng, att = _engine(E, "quantized_batched")
    eng.compute_all()
    T = eng.T
    before, ck, binfo = eng.stats(), eng.row_checksums(0, T), eng.batch_info()
    w = _matrix(T, T, seed=13)
    got = eng.table_load(weight=w)
    info = eng.table_load_info()
    assert info["tree"] > 0 and info["route"] > 0
    assert eng.stats() == before
    assert eng.batch_info() == binfo
    assert np.array_equal(eng.row_checksums(0, T), ck)
    eng.get_row(int(att[7]))
    assert eng.stats()["rowsComputed"] == before["rowsComputed"]
    _same(got, _reference(eng, 0, T, w))                      # (a path_load made afterwards: its own sums)
    eng.close()
    # rows not computed yet are computed first
    eng, _ = _engine(E, "quantized_batched")
    part = eng.table_load(10, 9, w[10:19])
    assert eng.stats()["rowsComputed"] == 9
    _same(part, _reference(eng, 10, 19, w[10:19], paths=False))
    eng.close()
