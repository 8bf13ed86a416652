"""GPU tests of the device graph build (shd_pe_create_built, pe_build.hip).

For every graph a host-built and a device-built engine are made from the same
description and must be indistinguishable: shd_pe_graph_digest equal entry for
entry (every HostGraph array, every DevGraph array as it sits on the device),
the same mode / isComplete / nArcs / deltaUsed, bit-identical table rows, and
a sample of rows bit-exact against the oracle.  The graphs are chosen for where
a build kernel can go wrong: bitmap word edges, rows longer than a workgroup,
empty and loop-only rows, loop rules, endpoint order, the heavy-degree
threshold, directed graphs (the IN CSR), and the two hand-offs."""
import os

import numpy as np
import pytest

from shdpe import generators as G
from shdpe.graph import Topology
from test_gpu_parity import _assert_rows_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("lat", "rel", "hops", "pred", "flags")


@pytest.fixture(scope="module")
def E():
    from shdpe import engine
    engine.load_library()
    return engine


def _all(n):
    return np.arange(n, dtype=np.int32)


def _sparse_directed():
    """random_sparse(400, 6) directed, both (a, b) and (b, a) for some pairs,
    and four vertices (400..403) with out-arcs only."""
    t = G.random_sparse(400, 6, seed=21, directed=True)
    have = set(zip(t.src.tolist(), t.dst.tolist()))
    rev = [(b, a) for a, b in list(have)[:40] if a != b and (b, a) not in have][:25]
    rng = np.random.default_rng(5)
    extra = [(400 + k, int(v)) for k in range(4) for v in rng.choice(400, 3, replace=False)]
    add = rev + extra
    src = np.concatenate([t.src, [a for a, _ in add]])
    dst = np.concatenate([t.dst, [b for _, b in add]])
    lat = np.concatenate([t.latency, rng.uniform(1.0, 100.0, len(add))])
    loss = np.concatenate([t.loss, rng.uniform(0.0, 0.05, len(add))])
    return Topology(404, True, src, dst, lat, loss, name="sparse_directed")


def _hub4097():
    """n = 4,097 (a last bitmap word of one bit): a sparse graph and a hub, the
    last vertex, adjacent to every other one -- its row sets every word."""
    t = G.random_sparse(4097, 6, seed=31)
    have = set(zip(np.minimum(t.src, t.dst).tolist(), np.maximum(t.src, t.dst).tolist()))
    others = [v for v in range(4096) if (v, 4096) not in have]
    rng = np.random.default_rng(6)
    src = np.concatenate([t.src, np.full(len(others), 4096)])       # given as (b, a), b > a
    dst = np.concatenate([t.dst, others])
    lat = np.concatenate([t.latency, rng.uniform(1.0, 100.0, len(others))])
    loss = np.concatenate([t.loss, rng.uniform(0.0, 0.05, len(others))])
    return Topology(4097, False, src, dst, lat, loss, name="hub4097")


def _empty_rows():
    """Isolated vertices (3, 7), a vertex whose only edges are loops (5)."""
    src = [0, 1, 2, 4, 6, 8, 9, 5, 5, 0, 10]
    dst = [1, 2, 4, 6, 8, 9, 10, 5, 5, 0, 11]
    lat = [3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 2.0, 1.5, 2.5, 1.0]
    loss = [0.01 * k for k in range(len(src))]
    return Topology(12, False, src, dst, lat, loss, name="empty_rows")


def _loops(directed):
    """Several loops on vertex 2 with equal minimum latencies (the newest of the
    minimum is the third of four), a slower newest loop, edges given as (b, a)
    with b > a."""
    src = [5, 4, 3, 2, 1, 2, 2, 2, 2, 0, 5, 3]
    dst = [0, 1, 2, 1, 0, 2, 2, 2, 2, 0, 4, 5]
    lat = [9.0, 8.0, 7.0, 6.0, 5.0, 5.0, 3.0, 3.0, 4.0, 2.0, 1.0, 2.0]
    loss = [0.0, 0.01, 0.02, 0.03, 0.04, 0.05, 0.06, 0.07, 0.08, 0.09, 0.1, 0.11]
    return Topology(6, directed, src, dst, lat, loss, vloss=np.array([0.0, np.nan, 0.02, 0.0, 1.0, 0.5]),
                    name="loops_dir" if directed else "loops")


def _heavy():
    """Vertex 0 at heavyDeg (64 arcs), vertex 100 just below it (63)."""
    src = [0] * 64 + [100] * 63
    dst = list(range(1, 65)) + list(range(101, 164))
    rng = np.random.default_rng(7)
    t = Topology(170, False, src + [64, 164], dst + [101, 165], rng.uniform(1.0, 50.0, 129),
                 rng.uniform(0.0, 0.05, 129), name="heavy")
    deg = np.bincount(np.concatenate([t.src, t.dst]), minlength=170)
    assert deg[0] == 64 and deg[100] == 63
    return t


def _shipped():
    return Topology.load_npz(os.path.join(ROOT, "tests", "golden", "shipped_topology.npz"), name="shipped")


# name -> (topology, attached, engine keywords)
_BUILDERS = {
    "sparse": lambda: (G.random_sparse(400, 6, seed=11, vloss=True), _all(400), {}),
    "sparse_directed": lambda: (_sparse_directed(), _all(404), {}),
    "complete257": lambda: (G.dense(257, seed=3), _all(257), {}),
    "complete257_minus1": lambda: (G.dense(257, seed=3, drop_edge=True), _all(257), {}),
    "shipped": lambda: (_shipped(), None, {}),
    "complete1100": lambda: (G.dense(1100, seed=4), G.sample_attached(1100, 96, seed=1), {}),
    "complete63": lambda: (G.dense(63, seed=5), _all(63), {}),
    "complete64": lambda: (G.dense(64, seed=5), _all(64), {}),
    "complete65": lambda: (G.dense(65, seed=5), _all(65), {}),
    "hub4097": lambda: (_hub4097(), np.concatenate([G.sample_attached(4096, 63, seed=2), [4096]]).astype(np.int32),
                        {}),
    "empty_rows": lambda: (_empty_rows(), _all(12), {}),
    "one_loop": lambda: (Topology(1, False, [0], [0], [3.0], [0.1], name="one_loop"), _all(1), {}),
    "two_no_edges": lambda: (Topology(2, False, [], [], [], [], name="two_no_edges"), _all(2), {}),
    "loops": lambda: (_loops(False), _all(6), {}),
    "loops_directed": lambda: (_loops(True), _all(6), {}),
    "heavy": lambda: (_heavy(), _all(170), {}),
    "batched": lambda: (G.random_sparse(400, 6, seed=12), _all(400), {"force_mode": 5}),
}
_CASES = {}


def _case(name):
    if name not in _CASES:
        top, att, kw = _BUILDERS[name]()
        if att is None:
            att = _all(top.n)
        _CASES[name] = (top, att, kw)
    return _CASES[name]


def _pair(E, top, att, **kw):
    host = E.Engine(top, att, graph_build=E.BUILD_HOST, **kw)
    dev = E.Engine(top, att, graph_build=E.BUILD_DEVICE, **kw)
    return host, dev


def _assert_same_graph(host, dev, ctx, shards=(0,)):
    for sh in shards:
        dh, dd = host.graph_digest(sh), dev.graph_digest(sh)
        assert dh.shape == dd.shape == (64,)
        bad = np.flatnonzero(dh != dd)
        assert bad.size == 0, f"{ctx} shard {sh}: digest entries {bad.tolist()} differ"
    sh_, sd = host.stats(), dev.stats()
    for k in ("mode", "isComplete", "nArcs", "deltaUsed"):
        assert sh_[k] == sd[k], (ctx, k, sh_[k], sd[k])


def _assert_same_tables(host, dev, ctx):
    host.compute_all()
    dev.compute_all()
    th, td = host.get_rows(0, host.T), dev.get_rows(0, dev.T)
    for k in FIELDS:
        a, b = th[k], td[k]
        if a.dtype == np.float64:
            a, b = a.view(np.int64), b.view(np.int64)
        assert np.array_equal(a, b), f"{ctx}: table field {k} differs"
    return td


def _assert_oracle_sample(oracle_mod, top, dev, table, ctx, count=6):
    og = oracle_mod.OracleGraph(top)
    idx = np.unique(np.linspace(0, dev.T - 1, min(count, dev.T)).astype(np.int64))
    if dev.stats()["mode"] == 2:
        # a complete graph is served from the edges (_topology_lookupDirectPath), as
        # test_gpu_parity.test_complete_graph_direct_rows checks it
        for i in idx:
            assert np.all(table["flags"][i] == 0x08), ctx
            for j, t in enumerate(dev.attached.tolist()):
                lat, rel = og.direct(int(dev.attached[i]), t)
                assert table["lat"][i][j] == lat and table["rel"][i][j] == rel, (ctx, i, j)
        return
    exp = og.rows(dev.attached[idx], dev.attached, threads=4)
    for j, i in enumerate(idx):
        _assert_rows_equal({k: table[k][i] for k in FIELDS}, {k: v[j] for k, v in exp.items()}, f"{ctx} row {i}")


@pytest.mark.parametrize("name", list(_BUILDERS))
def test_device_build_matches_host(E, oracle_mod, name):
    top, att, kw = _case(name)
    host, dev = _pair(E, top, att, **kw)
    try:
        bi = dev.build_info()
        assert bi["built"] == E.BUILD_DEVICE and bi["handedOff"] == 0 and bi["handOffWhy"] == 0, bi
        assert bi["deviceBytesPeak"] >= 24 * top.m and bi["msCreate"] > 0.0, bi
        hi = host.build_info()
        assert hi["built"] == E.BUILD_HOST and hi["handedOff"] == 0, hi
        assert np.array_equal(host.attached, dev.attached)
        _assert_same_graph(host, dev, name)
        if name == "batched":
            assert dev.stats()["batched"] == 1 and np.any(dev.graph_digest()[41:] != 0)
        table = _assert_same_tables(host, dev, name)
        _assert_oracle_sample(oracle_mod, top, dev, table, name)
    finally:
        host.close()
        dev.close()


def test_case_premises():
    """What the cases are there for (no engine)."""
    t, _, _ = _case("sparse_directed")
    pairs = set(zip(t.src.tolist(), t.dst.tolist()))
    assert sum((b, a) in pairs for a, b in pairs if a != b) >= 20
    assert not np.isin(np.arange(400, 404), t.dst).any() and np.isin(np.arange(400, 404), t.src).all()
    t, _, _ = _case("hub4097")
    assert np.count_nonzero((t.src == 4096) | (t.dst == 4096)) - 1 == 4096     # one loop
    assert np.any(t.src > t.dst)
    t, _, _ = _case("complete1100")
    assert t.m == 1100 * 1099 // 2 + 1100
    t, _, _ = _case("loops")
    assert np.count_nonzero((t.src == 2) & (t.dst == 2)) == 4


def test_complete_modes(E):
    """The complete graph is served directly, the one with an edge missing is not."""
    for name, complete, mode in (("complete257", 1, 2), ("complete257_minus1", 0, 3)):
        top, att, _ = _case(name)
        dev = E.Engine(top, att, graph_build=E.BUILD_DEVICE)
        st = dev.stats()
        dev.close()
        assert st["isComplete"] == complete and st["mode"] == mode, (name, st)


def test_multigraph_hands_off(E, oracle_mod):
    """The newest parallel edge slower than another of its group: the merge and
    latFold rules stay on the host."""
    top = G.with_slower_newest_edges(G.random_sparse(120, 4, seed=41), 0.3, seed=42)
    att = _all(120)
    host, dev = _pair(E, top, att)
    try:
        bi = dev.build_info()
        assert bi["built"] == E.BUILD_HOST and bi["handedOff"] == 1 and bi["handOffWhy"] == 1, bi
        _assert_same_graph(host, dev, "multigraph")
        assert host.graph_digest()[9] != 0                      # foldLat: a latFold graph
        table = _assert_same_tables(host, dev, "multigraph")
        _assert_oracle_sample(oracle_mod, top, dev, table, "multigraph")
    finally:
        host.close()
        dev.close()


def test_vertex_limit_hands_off(E, oracle_mod, monkeypatch):
    monkeypatch.setenv("SHDPE_BUILD_MAXN", "100")
    top, att, _ = _case("sparse")
    host, dev = _pair(E, top, att, debug_flags=E.DEBUG_ENV)
    try:
        bi = dev.build_info()
        assert bi["built"] == E.BUILD_HOST and bi["handedOff"] == 1 and bi["handOffWhy"] == 2, bi
        _assert_same_graph(host, dev, "maxn")
        table = _assert_same_tables(host, dev, "maxn")
        _assert_oracle_sample(oracle_mod, top, dev, table, "maxn")
    finally:
        host.close()
        dev.close()
    # without the debug flag the variable is not read
    dev = E.Engine(top, att, graph_build=E.BUILD_DEVICE)
    bi = dev.build_info()
    dev.close()
    assert bi["built"] == E.BUILD_DEVICE and bi["handedOff"] == 0, bi


def test_auto_follows_the_measured_threshold(E):
    """SHD_PE_BUILD_AUTO: the device build from the edge count
    profiles/create_device_build.json derives (a complete graph of 2,500
    vertices), the host build one edge below it."""
    import json
    thr = json.load(open(os.path.join(ROOT, "profiles", "create_device_build.json")))["auto_threshold_edges"]
    assert thr == 2500 * 2499 // 2 + 2500
    att = G.sample_attached(2500, 32, seed=3)
    for top, built in ((G.dense(2500, seed=3), E.BUILD_DEVICE), (G.dense(2500, seed=3, drop_edge=True), E.BUILD_HOST)):
        assert (top.m >= thr) == (built == E.BUILD_DEVICE)
        eng = E.Engine(top, att, graph_build=E.BUILD_AUTO)
        bi = eng.build_info()
        eng.close()
        assert bi["built"] == built and bi["handedOff"] == 0, (top.m, bi)


def test_two_shards_on_one_device(E):
    """The first shard adopts the built arrays, the second uploads HostGraph."""
    top, att, _ = _case("sparse")
    host, dev = _pair(E, top, att, devices=[0, 0])
    try:
        assert dev.build_info()["built"] == E.BUILD_DEVICE
        _assert_same_graph(host, dev, "sharded", shards=(0, 1))
        assert np.array_equal(dev.graph_digest(0), dev.graph_digest(1))
        _assert_same_tables(host, dev, "sharded")
    finally:
        host.close()
        dev.close()


@pytest.mark.parametrize("name", ["sparse", "sparse_directed", "complete257", "loops", "empty_rows"])
def test_direct_graph_helpers(E, name):
    top, att, kw = _case(name)
    host, dev = _pair(E, top, att, **kw)
    try:
        n = top.n
        rng = np.random.default_rng(3)
        src = np.concatenate([rng.integers(0, n, 400), top.src[:200], top.dst[:200], _all(n)[:50]]).astype(np.int32)
        dst = np.concatenate([rng.integers(0, n, 400), top.dst[:200], top.src[:200], _all(n)[:50]]).astype(np.int32)
        for a, b in zip(host.direct_paths(src, dst), dev.direct_paths(src, dst)):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), name
        for a, b in zip(host.self_paths(_all(n)), dev.self_paths(_all(n))):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), name
        assert np.array_equal(host.adjacent_pairs(src, dst), dev.adjacent_pairs(src, dst))
        assert host.is_complete_device() == dev.is_complete_device()
        for s, d in zip(src[:40].tolist(), dst[:40].tolist()):
            assert host.direct_path(s, d) == dev.direct_path(s, d)
        for v in range(min(n, 40)):
            assert host.self_path(v) == dev.self_path(v)
    finally:
        host.close()
        dev.close()


def _invalid(kind):
    t = G.random_sparse(50, 4, seed=51, vloss=True)
    src, dst, lat, loss, vloss = t.src.copy(), t.dst.copy(), t.latency.copy(), t.loss.copy(), t.vloss.copy()
    vloss[np.isnan(vloss)] = 0.0
    k = t.m // 2
    if kind == "latency0":
        lat[k] = 0.0
    elif kind == "latency_nan":
        lat[k] = np.nan
    elif kind == "loss1.5":
        loss[k] = 1.5
    elif kind == "endpoint_n":
        dst[k] = 50
    elif kind == "vloss_neg":
        vloss[7] = -0.1
    return Topology(50, False, src, dst, lat, loss, vloss=vloss, name=kind)


@pytest.mark.parametrize("kind", ["latency0", "latency_nan", "loss1.5", "endpoint_n", "vloss_neg"])
def test_invalid_inputs(E, kind):
    top = _invalid(kind)
    for build in (E.BUILD_HOST, E.BUILD_DEVICE):
        with pytest.raises(E.EngineError) as ei:
            E.Engine(top, _all(50), graph_build=build)
        assert ei.value.code == E.EINVAL, (kind, build)
    # the same description without the fault is accepted by the device build
    ok = G.random_sparse(50, 4, seed=51, vloss=True)
    eng = E.Engine(ok, _all(50), graph_build=E.BUILD_DEVICE)
    assert eng.build_info()["built"] == E.BUILD_DEVICE
    eng.close()
