"""shd_pe_fill_rowstore_ex / shd_topology_fill on the device against the host
sequence the header defines, built from existing calls: the engine's rows
through RowStore.store_rows (with the prefersDirectPaths adjacency from the
oracle's get_eid), then RowStore.store(isDirect=1) of the oracle's direct
paths for every ordered pair topology.c:2019-2021 serves from the edge
itself.  Bit-exact: same entries in the same direction, size, minimum
latency, per-row results."""
import os

import numpy as np
import pytest

from shdpe import generators as G
from shdpe.graph import Topology

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, D = 0x1, 0x2     # SHD_PE_FILL_PREFER_DIRECT, SHD_PE_FILL_DIRECT_PAIRS


@pytest.fixture(scope="module")
def E():
    from shdpe import engine
    assert (engine.FILL_PREFER_DIRECT, engine.FILL_DIRECT_PAIRS) == (P, D)
    return engine


def _drop_some_loops(top, seed):
    """Remove the self-loop of every 3rd vertex (missing (s,s) edges)."""
    rng = np.random.default_rng(seed)
    loops = np.flatnonzero(top.src == top.dst)
    drop = loops[rng.random(loops.shape[0]) < 0.33]
    keep = np.ones(top.m, bool)
    keep[drop] = False
    return Topology(n=top.n, directed=top.directed, src=top.src[keep], dst=top.dst[keep],
                    latency=top.latency[keep], loss=top.loss[keep], vloss=top.vloss,
                    name=top.name + "_someloops")


def _shipped():
    return Topology.load_npz(os.path.join(ROOT, "tests", "golden", "shipped_topology.npz"), name="shipped")


def _adjacency(og, att):
    """adj[p, q] = _topology_verticesAreAdjacent(att[p], att[q]) (the oracle)."""
    T = att.shape[0]
    adj = np.zeros((T, T), np.uint8)
    for p in range(T):
        s = int(att[p])
        for q in range(T):
            adj[p, q] = og.get_eid(s, int(att[q])) != -1
    return adj


class Case:
    """One engine with its table, adjacency and oracle, shared by the flag
    combinations of a graph (computed once, never modified)."""

    def __init__(self, E, oracle_mod, top, att, force=0, devices=None):
        self.E, self.top = E, top
        self.eng = E.Engine(top, att, force_mode=force, devices=devices)
        self.og = oracle_mod.OracleGraph(top)
        self.att = self.eng.attached
        self.adj = _adjacency(self.og, self.att)
        self.rows = None

    def reference(self, flags):
        """The contract with existing host calls -> (store, rowResult)."""
        E, eng, att, adj = self.E, self.eng, self.att, self.adj
        if self.rows is None:
            self.rows = eng.get_rows(0, eng.T)
        rows, C = self.rows, eng.is_complete
        ref = E.RowStore(self.top.n, att)
        rr = ref.store_rows(att, rows["lat"], rows["rel"], rows["flags"], is_complete=C,
                            adjacent=adj if flags & P else None)
        if flags & D and (C or flags & P):
            # ordered pairs in position order, p outer: C or (P and adjacent)
            for p, q in zip(*np.nonzero(np.ones_like(adj) if C else adj)):
                v = self.og.direct(int(att[p]), int(att[q]))     # None: no such edge
                if v is not None:
                    ref.store(int(att[p]), int(att[q]), 1, int(C), 0, v[0], v[1])
        return ref, np.asarray(rr, np.int32)

    def check(self, flags, st=None, eng=None):
        """Fill an empty store with `flags` and compare it with reference()."""
        E = self.E
        eng = eng or self.eng
        ref, rr = self.reference(flags)
        st = st or E.RowStore(self.top.n, self.att)
        res, _ = eng.fill_rowstore(st, fill_flags=flags)
        assert np.array_equal(res, rr)
        assert st.size() == ref.size() and st.min_latency() == ref.min_latency()
        items = sorted(st.items())
        assert items == sorted(ref.items())
        pos = {int(v): i for i, v in enumerate(self.att)}
        for s, d, lat, rel, isd, _ in items:
            if isd:
                assert (lat, rel) == self.og.direct(s, d), (s, d)
            else:
                assert not (flags & P and self.adj[pos[s], pos[d]]), (s, d)
        ref.close()
        return st, items

    def close(self):
        self.eng.close()


def _n_adjacent(adj):
    """adjacent attached pairs: unordered pairs with an arc either way + loops"""
    return int(np.triu(adj | adj.T).sum())


def test_sparse_with_dropped_loops_all_flag_words(E, oracle_mod):
    """Every flag word on an undirected graph with a third of its self-loops
    missing: P|D stores the edge for adjacent pairs, P alone leaves them out,
    D alone and 0 equal shd_pe_fill_rowstore; a missing loop leaves its
    diagonal slot empty."""
    top = _drop_some_loops(G.random_sparse(600, 5, seed=21, quantum=5.0), 2)
    c = Case(E, oracle_mod, top, np.arange(top.n, dtype=np.int32))
    assert _n_adjacent(c.adj) >= 100
    noloop = [int(v) for p, v in enumerate(c.att) if not c.adj[p, p]]
    assert len(noloop) >= 100
    plain = E.RowStore(top.n, c.att)
    c.eng.fill_rowstore(plain)
    plain_items = sorted(plain.items())
    got = {}
    for flags in (P | D, P, D, 0):
        st, got[flags] = c.check(flags)
        assert all(st.get(v, v) is None for v in noloop)
        with pytest.raises(E.EngineError) as ei:
            c.eng.fill_rowstore(st, fill_flags=flags)        # the store is no longer empty
        assert ei.value.code == E.EINVAL
        st.close()
    assert got[D] == plain_items and got[0] == plain_items
    ndirect = sum(1 for e in got[P | D] if e[4])
    assert ndirect == _n_adjacent(c.adj) and not any(e[4] for e in got[P])
    assert len(got[P]) == len(got[P | D]) - ndirect
    for bad in (0x4, 0x8 | P, -1):
        st = E.RowStore(top.n, c.att)
        with pytest.raises(E.EngineError) as ei:
            c.eng.fill_rowstore(st, fill_flags=bad)          # unknown flag bit
        assert ei.value.code == E.EINVAL and st.size() == 0
        st.close()
    plain.close()
    c.close()


def test_directed_reverse_keys_and_in_arcs(E, oracle_mod):
    """Directed, one-way arcs in both position orders.  An arc u -> v from an
    earlier to a later position refuses row u's Dijkstra entry, and row v's
    entry for u is stored under the reversed key only because the IN-arc
    bitmap says there is no arc v -> u; an arc from a later to an earlier
    position must not refuse the forward entry (the OUT bitmap is not the
    IN bitmap); pairs with arcs both ways are direct."""
    top = G.random_sparse(500, 3, seed=22, directed=True, vloss=True)
    c = Case(E, oracle_mod, top, np.arange(top.n, dtype=np.int32))
    oneway = c.adj.astype(bool) & ~c.adj.T.astype(bool)
    assert _n_adjacent(c.adj) >= 100 and int(np.tril(oneway, -1).sum()) >= 100
    assert int(np.triu(oneway, 1).sum()) >= 100
    st, items = c.check(P | D)
    pos = {int(v): i for i, v in enumerate(c.att)}
    assert sum(1 for s, d, *_r, isd, _pc in items if not isd and pos[s] > pos[d]) >= 100
    assert sum(1 for e in items if e[4]) >= 100
    st.close()
    c.close()


def test_newest_parallel_edge_slower(E, oracle_mod):
    """Multigraph whose newest parallel edge is not the fastest: the direct
    latency is the newest edge's (flat[]), not the group minimum."""
    top = G.with_slower_newest_edges(G.random_sparse(400, 6, seed=16, quantum=5.0), 0.4, seed=12)
    c = Case(E, oracle_mod, top, np.arange(top.n, dtype=np.int32))
    assert _n_adjacent(c.adj) >= 100
    st, _ = c.check(P | D)
    st.close()
    c.close()


def test_batched_relabelled_engine_with_hubs(E, oracle_mod):
    """The batched path relabels vertices by degree; hubs have more arcs than
    the workgroup has threads (the arc loop strides)."""
    top = G.power_law(20_000, m=3, seed=23)
    deg = np.bincount(np.concatenate([top.src, top.dst]), minlength=top.n)
    att = np.concatenate([G.sample_attached(top.n, 900, seed=4), np.argsort(-deg, kind="stable")[:8]])
    c = Case(E, oracle_mod, top, att.astype(np.int32), force=5)
    assert c.eng.stats()["batched"] == 1
    assert _n_adjacent(c.adj) >= 100 and int(deg[c.att].max()) > 256
    st, _ = c.check(P | D)
    st.close()
    c.close()


def test_dense_minus_one_edge(E, oracle_mod):
    """Almost every pair adjacent (full bitmap words); the one non-adjacent
    pair keeps its Dijkstra path."""
    top = G.dense(300, seed=2, drop_edge=True)
    c = Case(E, oracle_mod, top, np.arange(top.n, dtype=np.int32))
    assert not c.eng.is_complete and _n_adjacent(c.adj) >= 100
    st, items = c.check(P | D)
    nondirect = [e for e in items if not e[4]]
    assert 1 <= len(nondirect) <= 1 + top.n and len(items) - len(nondirect) == _n_adjacent(c.adj)
    st.close()
    c.close()


def test_complete_graphs_store_direct_pairs(E, oracle_mod):
    """Complete graphs: D stores every pair as a direct entry under (p <= q);
    without D nothing is stored.  On the shipped topology the mirror's fill
    equals a fresh reference cache queried over all ordered pairs in position
    order."""
    top = G.dense(80, seed=24)
    c = Case(E, oracle_mod, top, np.arange(top.n, dtype=np.int32))
    assert c.eng.is_complete and _n_adjacent(c.adj) >= 100
    st, items = c.check(D)
    pos = {int(v): i for i, v in enumerate(c.att)}
    assert len(items) == top.n * (top.n + 1) // 2
    assert all(isd and pos[s] <= pos[d] for s, d, *_r, isd, _pc in items)
    st.close()
    st, items = c.check(P | D)
    assert len(items) == top.n * (top.n + 1) // 2
    st.close()
    for flags in (P, 0):
        st, items = c.check(flags)
        assert not items
        st.close()
    c.close()

    top = _shipped()
    att = np.arange(top.n, dtype=np.int32)
    eng = E.Engine(top, att)
    assert eng.is_complete
    shim = E.TopologyShim(eng)
    shim.fill()
    ot = oracle_mod.OracleTopology(oracle_mod.OracleGraph(top), att)
    for s in att:
        for d in att:
            ot.get_latency(int(s), int(d))
    assert shim.cache_size == ot.cache_size >= 100 and shim.min_latency == ot.min_latency
    for s in att:
        for d in att:
            assert shim.cached(int(s), int(d)) == ot.cached(int(s), int(d)), (s, d)
    assert shim.rows_computed == 0
    shim.close()
    eng.close()


@pytest.mark.parametrize("T", [1, 65])
def test_tiny_tables(E, oracle_mod, T):
    """A single row, and a bitmap whose last word is partial."""
    top = G.random_sparse(130, 4, seed=3)
    c = Case(E, oracle_mod, top, np.arange(0, 2 * T, 2, dtype=np.int32))
    assert c.eng.T == T and c.adj.any()
    st, items = c.check(P | D)
    assert any(e[4] for e in items)
    st.close()
    c.close()


def test_sharded_engine(E, oracle_mod):
    """ENOTOWNED before gather(), then exactly the one-shard result."""
    top = G.power_law(6_000, m=3, seed=25)
    att = G.sample_attached(top.n, 700, seed=4)
    one = Case(E, oracle_mod, top, att, force=5)
    assert _n_adjacent(one.adj) >= 100
    eng = E.Engine(top, att, force_mode=5, devices=[0, 0])
    st = E.RowStore(top.n, eng.attached)
    with pytest.raises(E.EngineError) as ei:
        eng.fill_rowstore(st, prefers_direct=True, direct_pairs=True)
    assert ei.value.code == E.ENOTOWNED and st.size() == 0
    eng.gather()
    st, items = one.check(P | D, st=st, eng=eng)
    assert any(e[4] for e in items)
    st.close()
    eng.close()
    one.close()


def test_topology_mirror_fill(E, oracle_mod):
    """TopologyShim.fill() under prefersDirectPaths: afterwards no query
    computes a row, adjacent pairs return the edge, routability equals the
    reference's, and a second fill is refused."""
    top = G.random_sparse(600, 5, seed=21, quantum=5.0)
    att = np.arange(top.n, dtype=np.int32)
    eng = E.Engine(top, att)
    og = oracle_mod.OracleGraph(top)
    shim = E.TopologyShim(eng, prefers_direct=True)
    ot = oracle_mod.OracleTopology(og, att, prefers_direct=True)
    shim.fill()
    assert shim.cache_size > 0
    rng = np.random.default_rng(9)
    q = rng.integers(0, top.n, (3000, 2))
    q[:600, 1] = q[:600, 0]                             # (s, s) queries
    e = rng.integers(0, top.m, 800)
    q[600:1400] = np.stack([top.src[e], top.dst[e]], 1)   # adjacent pairs, both orders
    q[1000:1400] = q[1000:1400, ::-1]
    nadj = 0
    for s, d in q:
        s, d = int(s), int(d)
        lat, rel = shim.get_latency(s, d), shim.get_reliability(s, d)
        assert shim.is_routable(s, d) == ot.is_routable(s, d), (s, d)
        if og.get_eid(s, d) != -1:
            assert (lat, rel) == og.direct(s, d), (s, d)
            nadj += 1
    assert nadj >= 100
    assert shim.rows_computed == 0
    with pytest.raises(E.EngineError) as ei:
        shim.fill()
    assert ei.value.code == E.EINVAL
    shim.close()
    eng.close()
