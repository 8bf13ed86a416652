"""shd_pe_fill_rowstore_shards / shd_topology_fill_shards: the one-call
path-cache fill on a sharded in-process engine WITHOUT a gather, against the
contract of Case.reference in test_gpu_fill_direct.py (the host sequence
shd_rowstore_store_rows + direct pairs on rows read back with get_rows).
Logical shards on device 0; per fill: rowResult, size, minimum latency and the
sorted items.  The number of needs (slots whose reverse entry is another
shard's row) is derived here from the rows, the adjacency and
eng.shard_bounds() by the need rule and compared with the call's info."""
import numpy as np
import pytest

from shdpe import generators as G
from shdpe.graph import Topology
from test_gpu_fill_direct import Case, _drop_some_loops

pytestmark = pytest.mark.gpu

P, D = 0x1, 0x2
FAILED = 0x01 | 0x02


@pytest.fixture(scope="module")
def E():
    from shdpe import engine
    return engine


def need_masks(case, flags, bounds):
    """(need, answered_ok, provisional_direct) as T x T masks over slots
    (a, b), by the need rule: k = b - a > 0, row b behind the shard of row a,
    the forward entry not used, and (prefer-direct) no arc b -> a."""
    if case.rows is None:
        case.rows = case.eng.get_rows(0, case.eng.T)
    T = case.eng.T
    fail = (case.rows["flags"] & FAILED) != 0
    adj = case.adj.astype(bool)
    hi = np.empty(T, np.int64)
    for g in range(len(bounds) - 1):
        hi[bounds[g]:bounds[g + 1]] = bounds[g + 1]
    a, b = np.indices((T, T))
    behind = (b > a) & (b >= hi[:, None])
    C = case.eng.is_complete
    none = np.zeros((T, T), bool)
    if C:
        # a complete graph's direct table stores its entries as direct ones (D); Dijkstra rows
        # of a complete graph (force_mode) store no non-direct entry at all
        if not flags & D or case.eng.stats()["mode"] != 2:
            return none, none, none
        need = behind & fail
        return need, need & ~fail.T, none
    if flags & P:
        need = behind & (adj | fail) & ~adj.T
        return need, need & ~fail.T, (need & adj) if flags & D else none
    need = behind & fail
    return need, need & ~fail.T, none


def check_shards(case, eng, flags, need_budget=0):
    """Fill an empty store through the shard entry point, compare it with
    Case.reference and the info with the need rule -> (store, items, info)."""
    E = case.E
    ref, rr = case.reference(flags)
    st = E.RowStore(case.top.n, case.att)
    res, info = eng.fill_rowstore_shards(st, fill_flags=flags, need_budget=need_budget)
    assert np.array_equal(res, rr)
    assert st.size() == ref.size() and st.min_latency() == ref.min_latency()
    items = sorted(st.items())
    assert items == sorted(ref.items())
    ref.close()
    bounds = eng.shard_bounds()
    need, ok, _ = need_masks(case, flags, bounds)
    assert info["fromFullTable"] == 0 and info["shards"] == int((np.diff(bounds) > 0).sum())
    assert info["needs"] == int(need.sum()) and info["needsStored"] == int(ok.sum()), info
    assert (info["needRounds"] == 0) == (info["needs"] == 0)
    return st, items, info


def _entry(st, att, p, q):
    return st.get(int(att[p]), int(att[q]))


@pytest.fixture(scope="module")
def directed(E, oracle_mod):
    """The directed graph with one-way arcs and its 1-shard engine (rows,
    adjacency, oracle), shared and never modified."""
    top = G.random_sparse(500, 3, seed=22, directed=True, vloss=True)
    c = Case(E, oracle_mod, top, np.arange(top.n, dtype=np.int32))
    yield c
    c.close()


def test_directed_one_way_arcs_three_shards(E, directed):
    """Every flag word on three shards.  Under P a one-way arc u -> v from a
    lower to a higher position across shards refuses row u's entry and wants
    row v's: a need; P | D gives it the direct entry meanwhile."""
    c = directed
    eng = E.Engine(c.top, c.att, devices=[0, 0, 0])
    bounds = eng.shard_bounds()
    assert len(bounds) == 4 and (np.diff(bounds) > 0).all()
    got = {}
    for flags in (P | D, P, D, 0):
        st, got[flags], info = check_shards(c, eng, flags)
        need, ok, prov = need_masks(c, flags, bounds)
        if flags & P:
            assert info["needs"] >= 100 and info["needsStored"] > 0
            # an answered need is a non-direct entry under the reversed key, whatever the
            # pack had put there meanwhile (the edge, under P | D)
            assert (prov.sum() >= 100) == bool(flags & D)
            for a, b in zip(*np.nonzero(need & ok)):
                e = _entry(st, c.att, b, a)
                assert e is not None and not e[2] and _entry(st, c.att, a, b) is None
            # this graph is strongly connected: no reverse fold fails, so no need keeps its
            # provisional entry here (test_directed_sinks_... has those)
            assert not (need & ~ok).any()
        st.close()
    assert got[D] == got[0]
    eng.close()


def _with_sinks(top, first):
    """Vertices >= first lose their out-arcs (self-loops stay): arcs into them
    are one-way and nothing is reachable from them."""
    keep = (top.src < first) | (top.src == top.dst)
    return Topology(n=top.n, directed=True, src=top.src[keep], dst=top.dst[keep], latency=top.latency[keep],
                    loss=top.loss[keep], vloss=top.vloss, name=top.name + "_sinks")


def test_directed_sinks_failed_answers_keep_the_direct_entry(E, oracle_mod):
    """Answered-failed needs: the last 60 vertices are sinks, so an arc u ->
    sink from another shard is a need whose reverse fold is unreachable.
    Under P | D the slot keeps its provisional direct entry, under P it ends
    empty."""
    top = _with_sinks(G.random_sparse(400, 3, seed=22, directed=True, vloss=True), 340)
    c = Case(E, oracle_mod, top, np.arange(top.n, dtype=np.int32))
    eng = E.Engine(top, c.att, devices=[0, 0, 0])
    bounds = eng.shard_bounds()
    for flags in (P | D, P, 0):
        st, items, info = check_shards(c, eng, flags)
        need, ok, prov = need_masks(c, flags, bounds)
        failed = need & ~ok
        assert failed.sum() >= 100 and info["needs"] - info["needsStored"] == int(failed.sum())
        if flags & P:
            assert (failed & c.adj.astype(bool)).sum() >= 30 and ok.sum() > 0
        for a, b in zip(*np.nonzero(failed)):
            e = _entry(st, c.att, a, b)
            assert _entry(st, c.att, b, a) is None
            if prov[a, b]:
                assert e is not None and e[2] and e[:2] == c.og.direct(int(c.att[a]), int(c.att[b]))
            else:
                assert e is None
        st.close()
    eng.close()
    c.close()


def test_disconnected_undirected_two_shards(E, oracle_mod):
    """Two components, a third of the self-loops missing, plain flags: every
    cross-shard cross-component pair is a need, answered failed and left
    empty; a diagonal slot is never a need."""
    parts = [G.random_sparse(150, 4, seed=31, quantum=5.0), G.random_sparse(148, 4, seed=32, quantum=5.0)]
    n0 = parts[0].n
    top = Topology(n=n0 + parts[1].n, directed=False,
                   src=np.concatenate([parts[0].src, parts[1].src + n0]),
                   dst=np.concatenate([parts[0].dst, parts[1].dst + n0]),
                   latency=np.concatenate([parts[0].latency, parts[1].latency]),
                   loss=np.concatenate([parts[0].loss, parts[1].loss]), vloss=None, name="two_components")
    top = _drop_some_loops(top, 5)
    # attached order interleaves the components, so both shards hold rows of both
    att = np.arange(top.n, dtype=np.int32).reshape(2, -1).T.reshape(-1).copy()
    c = Case(E, oracle_mod, top, att)
    eng = E.Engine(top, att, devices=[0, 0])
    bounds = eng.shard_bounds()
    st, items, info = check_shards(c, eng, 0)
    need, ok, _ = need_masks(c, 0, bounds)
    comp = (c.att >= n0)
    cross = comp[:, None] != comp[None, :]
    a, b = np.indices(need.shape)
    behind = (b > a) & (a < bounds[1]) & (b >= bounds[1])
    assert (need & cross).sum() == (cross & behind).sum() >= 1000
    assert not (need & cross & ok).any() and not np.diag(need).any()
    noloop = [p for p in range(c.eng.T) if not c.adj[p, p]]
    assert len(noloop) >= 50 and all(_entry(st, c.att, p, p) is None for p in noloop)
    for p, q in zip(*np.nonzero(need & cross)):
        assert _entry(st, c.att, p, q) is None and _entry(st, c.att, q, p) is None
    st.close()
    eng.close()
    c.close()


def test_need_budget_rounds(E, directed):
    """64 bytes of budget hold two needs: many rounds, the same store."""
    c = directed
    eng = E.Engine(c.top, c.att, devices=[0, 0, 0])
    st1, items1, info1 = check_shards(c, eng, P | D)
    st2, items2, info2 = check_shards(c, eng, P | D, need_budget=64)
    assert info1["needRounds"] >= 1 and info2["needRounds"] > max(1, info1["needRounds"])
    assert info2["needs"] == info1["needs"] and items1 == items2
    st1.close()
    st2.close()
    eng.close()


@pytest.mark.parametrize("T", [1, 17, 65])
def test_tiny_tables_with_empty_shards(E, oracle_mod, T):
    top = G.random_sparse(130, 4, seed=3, directed=True)
    c = Case(E, oracle_mod, top, np.arange(0, 2 * T, 2, dtype=np.int32))
    eng = E.Engine(top, c.att, devices=[0] * 4)
    assert c.eng.T == T and len(eng.shard_bounds()) == 5
    if T == 1:
        assert (np.diff(eng.shard_bounds()) == 0).sum() == 3
    for flags in (P | D, 0):
        st, items, info = check_shards(c, eng, flags)
        assert items
        st.close()
    eng.close()
    c.close()


def test_dense_minus_one_edge_and_complete(E, oracle_mod):
    """Full bitmap words on two shards; a complete graph's direct table with D."""
    top = G.dense(300, seed=2, drop_edge=True)
    c = Case(E, oracle_mod, top, np.arange(top.n, dtype=np.int32))
    eng = E.Engine(top, c.att, devices=[0, 0])
    assert not eng.is_complete
    st, items, info = check_shards(c, eng, P | D)
    assert sum(1 for e in items if e[4]) >= 100
    st.close()
    eng.close()
    c.close()

    top = G.dense(80, seed=24)
    c = Case(E, oracle_mod, top, np.arange(top.n, dtype=np.int32))
    eng = E.Engine(top, c.att, devices=[0, 0])
    assert eng.is_complete
    st, items, info = check_shards(c, eng, D)
    assert len(items) == top.n * (top.n + 1) // 2 and all(e[4] for e in items)
    st.close()
    st, items, info = check_shards(c, eng, 0)
    assert not items
    st.close()
    eng.close()
    c.close()


def test_batched_engine_with_hubs(E, oracle_mod):
    top = G.power_law(20_000, m=3, seed=23)
    deg = np.bincount(np.concatenate([top.src, top.dst]), minlength=top.n)
    att = np.concatenate([G.sample_attached(top.n, 900, seed=4), np.argsort(-deg, kind="stable")[:8]])
    c = Case(E, oracle_mod, top, att.astype(np.int32), force=5)
    eng = E.Engine(top, c.att, force_mode=5, devices=[0, 0])
    assert eng.stats()["batched"] == 1 and int(deg[c.att].max()) > 256
    st, items, info = check_shards(c, eng, P | D)
    assert sum(1 for e in items if e[4]) >= 100
    st.close()
    eng.close()
    c.close()


def test_equivalences_and_refusals(E, directed):
    c = directed
    T = c.eng.T
    ex = E.RowStore(c.top.n, c.att)
    c.eng.fill_rowstore(ex, fill_flags=P | D)
    ex_items = sorted(ex.items())
    ex.close()
    # one shard: the _ex path
    st = E.RowStore(c.top.n, c.att)
    res, info = c.eng.fill_rowstore_shards(st, fill_flags=P | D)
    assert info["fromFullTable"] == 1 and info["shards"] == 1 and info["needs"] == 0 and info["needRounds"] == 0
    assert sorted(st.items()) == ex_items
    for bad_flags, store in ((0x4, None), (P | D, st)):          # unknown bit; non-empty store
        s2 = store or E.RowStore(c.top.n, c.att)
        with pytest.raises(E.EngineError) as ei:
            c.eng.fill_rowstore_shards(s2, fill_flags=bad_flags)
        assert ei.value.code == E.EINVAL
        if store is None:
            assert s2.size() == 0
            s2.close()
    st.close()
    # two shards, not gathered: _ex refuses, the shard fill needs no full table
    eng = E.Engine(c.top, c.att, devices=[0, 0])
    st = E.RowStore(c.top.n, c.att)
    with pytest.raises(E.EngineError) as ei:
        eng.fill_rowstore(st, fill_flags=P | D)
    assert ei.value.code == E.ENOTOWNED and st.size() == 0
    for bad in (0x4, 0x8 | P, -1):
        with pytest.raises(E.EngineError) as ei:
            eng.fill_rowstore_shards(st, fill_flags=bad)
        assert ei.value.code == E.EINVAL and st.size() == 0
    res, info = eng.fill_rowstore_shards(st, fill_flags=P | D)
    full_table_bytes = T * T * (8 + 8 + 4 + 4 + 1)
    assert info["fromFullTable"] == 0 and 0 < info["deviceBytesPeak"] < full_table_bytes
    assert sorted(st.items()) == ex_items
    with pytest.raises(E.EngineError) as ei:
        eng.fill_rowstore_shards(st, fill_flags=P | D)           # no longer empty
    assert ei.value.code == E.EINVAL
    st.close()
    st = E.RowStore(c.top.n, c.att)
    with pytest.raises(E.EngineError) as ei:
        eng.fill_rowstore(st, fill_flags=P | D)                  # still not gathered
    assert ei.value.code == E.ENOTOWNED
    # gathered: the _ex path again
    eng.gather()
    res, info = eng.fill_rowstore_shards(st, fill_flags=P | D)
    assert info["fromFullTable"] == 1 and info["shards"] == 1 and sorted(st.items()) == ex_items
    st.close()
    eng.close()
    # one engine of two processes': the other rows' store is not here
    eng = E.Engine(c.top, c.att, shard_index=0, shard_count=2)
    st = E.RowStore(c.top.n, c.att)
    with pytest.raises(E.EngineError) as ei:
        eng.fill_rowstore_shards(st, fill_flags=P | D)
    assert ei.value.code == E.ENOTOWNED and st.size() == 0
    st.close()
    eng.close()


def test_topology_mirror_fill_shards(E, oracle_mod):
    """TopologyShim.fill_shards() on two shards under prefersDirectPaths, as
    test_topology_mirror_fill: no query computes a row afterwards."""
    top = G.random_sparse(600, 5, seed=21, quantum=5.0)
    att = np.arange(top.n, dtype=np.int32)
    eng = E.Engine(top, att, devices=[0, 0])
    og = oracle_mod.OracleGraph(top)
    shim = E.TopologyShim(eng, prefers_direct=True)
    ot = oracle_mod.OracleTopology(og, att, prefers_direct=True)
    info = shim.fill_shards()
    assert shim.cache_size > 0 and info["fromFullTable"] == 0 and info["shards"] == 2
    rng = np.random.default_rng(9)
    q = rng.integers(0, top.n, (3000, 2))
    q[:600, 1] = q[:600, 0]
    e = rng.integers(0, top.m, 800)
    q[600:1400] = np.stack([top.src[e], top.dst[e]], 1)
    q[1000:1400] = q[1000:1400, ::-1]
    nadj = 0
    for s, d in q:
        s, d = int(s), int(d)
        lat, rel = shim.get_latency(s, d), shim.get_reliability(s, d)
        assert shim.is_routable(s, d) == ot.is_routable(s, d), (s, d)
        if og.get_eid(s, d) != -1:
            assert (lat, rel) == og.direct(s, d), (s, d)
            nadj += 1
    assert nadj >= 100 and shim.rows_computed == 0
    with pytest.raises(E.EngineError) as ei:
        shim.fill_shards()
    assert ei.value.code == E.EINVAL
    shim.close()
    eng.close()


def test_distinct_devices(E, directed):
    """One shard per device: the image takes DMA from both.  Skipped with < 2 GPUs."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs >= 2 GPUs (one device per shard)")
    c = directed
    eng = E.Engine(c.top, c.att, devices=[0, 1])
    st, items, info = check_shards(c, eng, P | D)
    assert info["needs"] >= 100 and info["needsStored"] > 0
    st.close()
    eng.close()
