"""GPU tests of the all-pairs load's parent tier
(shd_pe_table_load_set_parent_tier, k_tree_load_parents): the sums against
shd_pe_path_load on the explicit request list and, where stated, against numpy
over the paths shd_pe_get_paths returns, exactly; on the per-row sparse kernel
in every kind of graph, on the shapes where the kernel can go wrong (deep
chains, one hub, one source, few destinations), across groups and reused
scratch slots, with every kind of weight, over the tie slots of the batched
engine, with the hand-on injected, without side effects and across shards."""
import numpy as np
import pytest

from shdpe import generators as G
from shdpe.graph import Topology
from test_gpu_parity import _chain
from test_gpu_path_load import _engine, _sum_paths, _usum
from test_gpu_paths import CASES, E, _Oracle  # noqa: F401  (E: the fixture)
from test_gpu_table_load import _chain_sums, _matrix, _pairs, _reference, _same

pytestmark = pytest.mark.gpu

U64 = np.uint64
SWITCHES = ("SHDPE_TLOAD_TREE", "SHDPE_TLOAD_CORRUPT", "SHDPE_BATCH_GRID", "SHDPE_PATHS_GROUP",
            "SHDPE_PATHS_FAST", "SHDPE_TIE_SLOTS", "SHDPE_TIE_CORRUPT")


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


def _env_engine(E, monkeypatch, top, att, env, force_mode=1, **kw):
    for k, v in env.items():
        assert k in SWITCHES, k
        monkeypatch.setenv(k, str(v))
    return _on(E.Engine(top, att, force_mode=force_mode, debug_flags=E.DEBUG_ENV | E.DEBUG_COUNTERS, **kw))


def _exact_rows(E, eng):
    return int(np.count_nonzero(np.any(eng.get_rows(0, eng.T)["flags"] & E.F_EXACT, axis=1)))


# ---- 1. the sparse modes --------------------------------------------------------

def _directed_sparse(E):
    """The graph of test_gpu_table_load's _directed_with_unreachable (one more
    vertex with an out-arc only, attached: no other source reaches it) on the
    per-row sparse kernel."""
    base = CASES["directed"][0]()
    n = base.n
    top = Topology(n=n + 1, directed=True, src=np.concatenate([base.src, [n]]), dst=np.concatenate([base.dst, [0]]),
                   latency=np.concatenate([base.latency, [3.0]]), loss=np.concatenate([base.loss, [0.0]]))
    att = np.concatenate([np.arange(0, n, 3), [n]]).astype(np.int32)
    return E.Engine(top, att, force_mode=0), att


@pytest.mark.parametrize("name", ["tiefree", "quantized", "directed", "vloss"])
def test_sparse_modes(E, name):
    eng, att = _directed_sparse(E) if name == "directed" else _engine(E, name)
    _on(eng)
    T = eng.T
    w = _matrix(T, T)
    assert np.any(w == 0)
    ref = _reference(eng, 0, T, w)
    got = eng.table_load(weight=w)
    info = eng.table_load_info()
    print(name, info, got["totals"])
    _same(got, ref)
    _one_route_each(info, T)
    assert info["tree"] == 0 and info["direct"] == 0
    assert info["parents"] > 0 and info["parent_claimed"] > 0
    if name == "tiefree":
        assert info["parents"] == T and info["route"] == 0
    if name == "quantized":
        assert info["tie"] >= 1 and info["handed_on"] == 0
        assert info["route"] <= _exact_rows(E, eng)
    if name == "directed":
        assert int(got["totals"][3]) > 0
    eng.close()


# ---- 2. off by default ----------------------------------------------------------

def test_off_by_default(E):
    eng, att = _engine(E, "quantized")
    T = eng.T
    w = _matrix(T, T, seed=2)
    ref = _reference(eng, 0, T, w, paths=False)

    def off():
        got = eng.table_load(weight=w)
        info = eng.table_load_info()
        _same(got, ref)
        assert info["parents"] == info["tie"] == info["parent_claimed"] == info["parent_atomics"] == 0
        assert info["route"] == T and info["tree"] == 0 and info["handed_on"] == 0

    off()
    _on(eng)
    _same(eng.table_load(weight=w), ref)
    assert eng.table_load_info()["parents"] > 0
    eng.set_table_load_parent_tier(False)
    off()
    eng.close()


def test_paths_fast_switch_turns_it_off(E, monkeypatch):
    make = CASES["tiefree"][0]
    top = make()
    att = np.arange(0, top.n, 3, dtype=np.int32)
    eng = _env_engine(E, monkeypatch, top, att, {"SHDPE_PATHS_FAST": 0})
    got = eng.table_load(0, 5)
    info = eng.table_load_info()
    _same(got, _reference(eng, 0, 5, None, paths=False))
    assert info["parents"] == 0 and info["route"] == 5
    eng.close()


# ---- 3. against the oracle ------------------------------------------------------

def test_against_oracle(E, oracle_mod):
    """60 sources of the tie-free graph on the sparse kernel, against igraph's paths."""
    top = CASES["tiefree"][0]()
    att = np.arange(0, top.n, 3, dtype=np.int32)
    eng = _on(E.Engine(top, att, force_mode=1))
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


# ---- 4. shapes where the kernel can go wrong ------------------------------------

@pytest.mark.parametrize("n", [257, 2000])
def test_chain(E, n):
    """A path graph with every vertex attached: the tree of an end is n - 1 deep
    and its leaves-first sum is one thread's loop; a source in the middle has two
    such branches."""
    top = _chain(n, seed=n)
    first = [0, n - 1, n // 2]
    att = np.array(first + [v for v in range(n) if v not in first], np.int32)
    eng = _on(E.Engine(top, att, force_mode=1))
    for lo, hi in [(0, 3)] + ([(0, n)] if n == 257 else []):
        w = _matrix(hi - lo, n, seed=n + hi)
        got = eng.table_load(lo, hi - lo, w)
        info = eng.table_load_info()
        print(n, (lo, hi), info)
        _same(got, _reference(eng, lo, hi, w, paths=n == 257))
        vertex, up, down = _chain_sums(n, att, lo, hi, w)
        assert np.array_equal(got["vertex"], vertex)
        for v in (0, n // 3, n - 2):
            assert int(got["arc"][eng.find_arc(v, v + 1)]) == int(up[v])
            assert int(got["arc"][eng.find_arc(v + 1, v)]) == int(down[v])
        assert info["parents"] == hi - lo and info["route"] == 0
        assert info["parent_claimed"] >= (hi - lo) * n * 9 // 10   # (a weight-0 leaf end is not claimed)
    eng.close()


def test_star(E):
    """A star of 1,000 leaves: from a leaf the hub's pending word takes 999 adds
    and its sum as many; from the hub the source's does."""
    L = 1000
    leaves = np.arange(1, L + 1)
    src = np.concatenate([np.zeros(L, np.int64), np.arange(L + 1)])
    dst = np.concatenate([leaves, np.arange(L + 1)])
    rng = np.random.default_rng(5)
    top = Topology(L + 1, False, src, dst, np.concatenate([rng.uniform(1.0, 2.0, L), np.ones(L + 1)]),
                   np.zeros(src.shape[0]))
    att = np.arange(L + 1, dtype=np.int32)
    eng = _on(E.Engine(top, att, force_mode=1))
    w = _matrix(2, L + 1, seed=3)
    got = eng.table_load(0, 2, w)                             # the hub, then leaf 1
    info = eng.table_load_info()
    _same(got, _reference(eng, 0, 2, w))
    assert int(got["vertex"][0]) == _usum(w[0]) + _usum(w[1]) - int(w[1, 1])
    assert info["parents"] == 2 and info["route"] == 0
    eng.close()


def test_one_attached_vertex(E):
    top = G.random_sparse(300, 4, seed=2)
    eng = _on(E.Engine(top, np.array([17], np.int32), force_mode=1))
    w = np.array([[5]], U64)
    got = eng.table_load(weight=w)
    info = eng.table_load_info()
    _same(got, _reference(eng, 0, 1, w))
    assert int(got["vertex"][17]) == 5 and _usum(got["vertex"]) == 5 and not got["arc"].any()
    assert info["parents"] == 1 and info["parent_claimed"] == 1
    eng.close()


def test_few_destinations(E):
    """12 attached vertices of 2,000: most of the scratch slot is never claimed."""
    top = G.random_sparse(2000, 5, seed=23)
    att = np.arange(5, 2000, 170, dtype=np.int32)
    assert att.shape[0] == 12
    eng = _on(E.Engine(top, att, force_mode=1))
    w = _matrix(12, 12, seed=4)
    got = eng.table_load(weight=w)
    info = eng.table_load_info()
    _same(got, _reference(eng, 0, 12, w))
    assert info["parents"] == 12 and info["route"] == 0
    assert 12 <= info["parent_claimed"] < 12 * 2000 // 4
    eng.close()


# ---- 5. groups and slot reuse ---------------------------------------------------

@pytest.mark.parametrize("group,grid", [(3, 0), (1, 0), (0, 2), (3, 1)])
def test_groups_and_slot_reuse(E, monkeypatch, group, grid):
    """40 sources in groups of 3 or 1 (the scratch slots of the row kernel are
    overwritten by the next group), and on 2 or 1 workgroups of the tree kernel
    (a workgroup's slot is reused for its next source)."""
    top = G.random_sparse(500, 5, seed=21)
    att = np.arange(0, 40 * 12, 12, dtype=np.int32)
    env = {}
    if group:
        env["SHDPE_PATHS_GROUP"] = group
    if grid:
        env["SHDPE_BATCH_GRID"] = grid
    eng = _env_engine(E, monkeypatch, top, att, env)
    w = _matrix(40, 40, seed=group + grid)
    got = eng.table_load(weight=w)
    info = eng.table_load_info()
    _same(got, _reference(eng, 0, 40, w))
    assert info["parents"] == 40 and info["route"] == 0
    assert 0 < info["parent_atomics"] <= 2 * info["parent_claimed"]
    eng.close()


# ---- 6. weights -----------------------------------------------------------------

def test_weights(E):
    eng, att = _engine(E, "tiefree")
    _on(eng)
    T = eng.T
    ones = eng.table_load(weight=np.ones((T, T), U64))
    none = eng.table_load()
    assert eng.table_load_info()["parents"] == T
    _same(none, ones)
    _same(none, _reference(eng, 0, T, None, paths=False))
    # a leading dimension past T, garbage behind the rows
    wide = _matrix(T, T, seed=5, ld=T + 5)
    _same(eng.table_load(weight=wide), _reference(eng, 0, T, wide, paths=False))
    # sums that wrap
    top_w = np.full((40, T), 2 ** 64 - 1, U64)
    got = eng.table_load(3, 40, top_w)
    assert eng.table_load_info()["parents"] == 40
    _same(got, _reference(eng, 3, 43, top_w, paths=False))
    assert int(got["vertex"].max()) > 2 ** 63                # (-k mod 2^64)
    # a sub-range, one row, no row
    w = _matrix(T, T, seed=6)
    w[17] = 0
    got = eng.table_load(5, 23, w[5:28])
    assert eng.table_load_info()["parents"] == 23
    _same(got, _reference(eng, 5, 28, w[5:28], paths=False))
    one = eng.table_load(T - 1, 1, w[T - 1:])
    assert eng.table_load_info()["parents"] == 1
    _same(one, _reference(eng, T - 1, T, w[T - 1:], paths=False))
    none = eng.table_load(9, 0)
    assert not none["arc"].any() and not none["vertex"].any() and not none["totals"].any()
    info = eng.table_load_info()
    assert info["parents"] == info["tie"] == info["route"] == 0
    eng.close()


# ---- 7. tie slots on the batched engine -----------------------------------------

@pytest.mark.parametrize("name", ["quantized_batched", "powerlaw_batched"])
def test_batched_tie_slots(E, name):
    eng, att = _engine(E, name)
    T = eng.T
    w = _matrix(T, T, seed=14)
    off = eng.table_load(weight=w)
    ioff = eng.table_load_info()
    assert ioff["tie"] == 0 and ioff["parents"] == 0 and ioff["route"] > 0
    _on(eng)
    got = eng.table_load(weight=w)
    info = eng.table_load_info()
    print(name, ioff, info)
    for key in ("arc", "vertex", "totals"):
        assert np.array_equal(got[key], off[key]), key
    _same(got, _reference(eng, 0, T, w, paths=False))
    _one_route_each(info, T)
    assert info["tie"] >= 1 and info["tree"] == ioff["tree"] > 0 and info["parents"] == 0
    assert info["handed_on"] == 0 and info["route"] == ioff["route"] - info["tie"]
    assert info["route"] <= _exact_rows(E, eng) - info["tie"]   # the rows left to the full emulation
    eng.close()


def test_batched_without_tie_slots(E, monkeypatch):
    make = CASES["quantized_batched"][0]
    top = make()
    att = np.arange(0, top.n, 3, dtype=np.int32)
    eng = _env_engine(E, monkeypatch, top, att, {"SHDPE_TIE_SLOTS": 0}, force_mode=5)
    T = eng.T
    w = _matrix(T, T, seed=14)
    got = eng.table_load(weight=w)
    info = eng.table_load_info()
    _same(got, _reference(eng, 0, T, w, paths=False))
    _one_route_each(info, T)
    assert info["tie"] == 0 and info["tree"] > 0 and info["route"] > 0
    eng.close()


# ---- 8. hand-on by injection ----------------------------------------------------

@pytest.mark.parametrize("value", [1, 2, 3])
def test_hand_on_sparse(E, monkeypatch, value):
    top = CASES["tiefree"][0]()
    att = np.arange(0, top.n, 3, dtype=np.int32)
    eng = _env_engine(E, monkeypatch, top, att, {"SHDPE_TLOAD_CORRUPT": value})
    w = _matrix(50, eng.T, seed=9)
    got = eng.table_load(4, 50, w)
    info = eng.table_load_info()
    _same(got, _reference(eng, 4, 54, w, paths=False))
    _one_route_each(info, 50)
    assert info["handed_on"] == 1 and info["route"] == 1 and info["parents"] == 49
    assert eng.path_load_info()["entries"] > 0            # (the request route served it)
    eng.close()


def test_hand_on_batched_tie_row(E, monkeypatch):
    """SHDPE_TLOAD_CORRUPT=1 on a range whose first source is a tie row with a slot."""
    make = CASES["quantized_batched"][0]
    top = make()
    att = np.arange(0, top.n, 3, dtype=np.int32)
    eng = _on(E.Engine(top, att, force_mode=5))
    T = eng.T
    exact = np.flatnonzero(np.any(eng.get_rows(0, T)["flags"] & E.F_EXACT, axis=1))
    start = -1
    for p in exact[:12]:
        eng.table_load(int(p), 1)
        if eng.table_load_info()["tie"] == 1:
            start = int(p)
            break
    eng.close()
    assert start >= 0
    count = min(30, T - start)
    eng = _env_engine(E, monkeypatch, top, att, {"SHDPE_TLOAD_CORRUPT": 1}, force_mode=5)
    w = _matrix(count, T, seed=10)
    got = eng.table_load(start, count, w)
    info = eng.table_load_info()
    _same(got, _reference(eng, start, start + count, w, paths=False))
    _one_route_each(info, count)
    assert info["handed_on"] == 1 and info["route"] >= 1
    eng.close()


def test_failed_tie_slot_gives_no_sum(E, monkeypatch):
    """SHDPE_TIE_CORRUPT spoils a slot's exported distances: the emulation's
    check sets its threshold to NaN, and the kernel hands the row on itself."""
    top = CASES["quantized"][0]()
    att = np.arange(0, top.n, 3, dtype=np.int32)
    eng = _env_engine(E, monkeypatch, top, att, {"SHDPE_TIE_CORRUPT": 1}, force_mode=0)
    T = eng.T
    w = _matrix(T, T, seed=11)
    got = eng.table_load(weight=w)
    info = eng.table_load_info()
    print(info)
    _same(got, _reference(eng, 0, T, w, paths=False))
    _one_route_each(info, T)
    assert info["handed_on"] >= 1 and info["route"] >= info["handed_on"]
    eng.close()


# ---- 9. no side effects ---------------------------------------------------------

def test_no_side_effects(E):
    eng, att = _engine(E, "quantized")
    _on(eng)
    eng.compute_all()
    T = eng.T
    before, ck, binfo = eng.stats(), eng.row_checksums(0, T), eng.batch_info()
    w = _matrix(T, T, seed=13)
    got = eng.table_load(weight=w)
    info = eng.table_load_info()
    assert info["parents"] > 0 and info["tie"] > 0
    assert eng.stats() == before
    assert eng.batch_info() == binfo
    assert np.array_equal(eng.row_checksums(0, T), ck)
    _same(got, _reference(eng, 0, T, w, paths=False))
    eng.close()


# ---- 10. two local shards -------------------------------------------------------

def test_two_local_shards(E):
    eng, att = _engine(E, "quantized")
    T = eng.T
    w = _matrix(T, T, seed=12)
    ref = _reference(eng, 0, T, w, paths=False)
    eng.close()
    eng, _ = _engine(E, "quantized", devices=[0, 0])
    _on(eng)
    bounds = eng.shard_bounds()
    assert len(bounds) == 3 and 0 < bounds[1] < T
    lo, hi = int(bounds[1]) - 20, int(bounds[1]) + 30
    got = eng.table_load(weight=w)
    info = eng.table_load_info()
    part = eng.table_load(lo, hi - lo, w[lo:hi])
    pinfo = eng.table_load_info()
    _same(part, _reference(eng, lo, hi, w[lo:hi], paths=False))
    eng.close()
    _same(got, ref)
    _one_route_each(info, T)
    _one_route_each(pinfo, hi - lo)
    assert info["parents"] > 0 and pinfo["parents"] > 0
