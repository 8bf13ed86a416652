"""GPU tests of the batched path extraction (shd_pe_get_paths): every path
against the oracle's igraph Dijkstra, the hop attributes against the edge
igraph_get_eid picks, per-request failures, the sizing protocol, grouping /
chunking, sharding, and the absence of side effects on the table."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
from shdpe import generators as G
from shdpe.graph import Topology

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    from shdpe import engine
    engine.load_library()
    return engine


def _oracle_path(top, raw, s, t):
    """igraph's path s -> t from the oracle's raw Dijkstra of s (og.raw:
    distances, parent edge ids); None when t was not reached."""
    dist, par, _ = raw
    if dist[t] < 0:
        return None
    path, v = [int(t)], int(t)
    while v != s:
        e = int(par[v]) - 1
        assert e >= 0, "unreached"
        a, b = int(top.src[e]), int(top.dst[e])
        v = a if (top.directed or b == v) else b
        path.append(v)
    return path[::-1]


class _Oracle:
    """One raw Dijkstra per source, shared by every request of a case."""

    def __init__(self, oracle_mod, top, att):
        self.top, self.att = top, np.asarray(att, np.int32)
        self.og = oracle_mod.OracleGraph(top)
        self._raw = {}

    def path(self, s, t):
        s, t = int(s), int(t)
        if s == t:
            return [s]
        if s not in self._raw:
            self._raw[s] = self.og.raw(s, self.att)
        return _oracle_path(self.top, self._raw[s], s, t)


def _requests(att, n_src=40, n_dst=8, seed=5):
    """n_src sources x n_dst destinations; src == dst and repeated pairs included."""
    rng = np.random.default_rng(seed)
    att = np.asarray(att, np.int32)
    srcs = rng.choice(att, min(n_src, att.shape[0]), replace=False)
    src, dst = [], []
    for k, s in enumerate(srcs):
        d = rng.choice(att, n_dst)
        if k % 4 == 0:
            d[0] = s                      # the 1-vertex path
        if k % 5 == 0:
            d[-1] = d[1]                  # the same pair twice in one source
        src += [s] * n_dst
        dst += list(d)
    src += src[:5]                        # ... and at the far end of the call
    dst += dst[:5]
    return np.asarray(src, np.int32), np.asarray(dst, np.int32)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _check_against_oracle(E, eng, orc, src, dst, fold):
    top, og = orc.top, orc.og
    offsets, verts, status, hl, hr = eng.get_paths(src, dst, hops=True)
    assert offsets[0] == 0 and offsets.shape[0] == src.shape[0] + 1
    pos = {int(v): k for k, v in enumerate(eng.attached)}
    rows = {}
    for i in range(src.shape[0]):
        s, t = int(src[i]), int(dst[i])
        exp = orc.path(s, t)
        a, b = int(offsets[i]), int(offsets[i + 1])
        if exp is None:
            assert status[i] == E.EUNREACHABLE and a == b, (i, s, t)
            continue
        assert status[i] == 0, (i, s, t, status[i])
        assert verts[a:b].tolist() == exp, (i, s, t)
        assert hl[a] == 0.0 and hr[a] == 0.0
        if s == t:
            continue
        if s not in rows:
            rows[s] = eng.get_row(s)
        row = rows[s]
        assert b - a == row["hops"][pos[t]] + 1, (i, s, t)
        eids = [og.get_eid(exp[k - 1], exp[k]) for k in range(1, len(exp))]
        assert min(eids) >= 0
        assert np.array_equal(_bits(hl[a + 1:b]), _bits(top.latency[eids])), (i, s, t)
        assert np.array_equal(_bits(hr[a + 1:b]), _bits(1.0 - top.loss[eids])), (i, s, t)
        if fold and not (row["flags"][pos[t]] & E.F_ZEROLAT):
            acc = 0.0
            for x in hl[a + 1:b]:
                acc = acc + float(x)
            assert _bits([acc])[0] == _bits([row["lat"][pos[t]]])[0], (i, s, t)
    return offsets, verts, status, hl, hr


CASES = {
    # name: (graph, attached, forceMode, fold check)
    "tiefree": (lambda: G.random_sparse(800, 5, seed=34), None, 0, True),
    "tiefree_batched": (lambda: G.random_sparse(800, 5, seed=34), None, 5, True),
    "quantized": (lambda: G.random_sparse(800, 5, seed=32, quantum=0.5), None, 0, False),
    "quantized_batched": (lambda: G.random_sparse(800, 5, seed=32, quantum=0.5), None, 5, False),
    "directed": (lambda: G.random_sparse(700, 5, seed=31, directed=True), None, 0, False),
    "directed_batched": (lambda: G.random_sparse(700, 5, seed=31, directed=True), None, 5, False),
    "powerlaw_batched": (lambda: G.power_law(3000, 3, seed=33, quantum=0.25), None, 5, False),
    "vloss": (lambda: G.random_sparse(600, 5, seed=35, vloss=True), None, 0, False),
    "latfold": (lambda: G.with_slower_newest_edges(G.random_sparse(60, 4, seed=2), 0.4, seed=4), None, 0, True),
    "dense": (lambda: G.dense(300, seed=3, drop_edge=True), None, 4, False),
}


def _case(name):
    make, att, force, fold = CASES[name]
    top = make()
    att = np.arange(0, top.n, 3, dtype=np.int32) if att is None else att
    return top, att, force, fold


@pytest.mark.parametrize("name", list(CASES))
def test_paths_match_oracle(E, oracle_mod, name):
    """Every request against igraph's path, its length against the table's
    hops, every hop's latency / reliability against igraph_get_eid's edge."""
    top, att, force, fold = _case(name)
    eng = E.Engine(top, att, force_mode=force)
    orc = _Oracle(oracle_mod, top, eng.attached)
    src, dst = _requests(att)
    assert np.any(src == dst) and src.shape[0] > np.unique(np.stack([src, dst]), axis=1).shape[1]
    _check_against_oracle(E, eng, orc, src, dst, fold)
    info = eng.paths_info()
    n_uniq = np.unique(src[src != dst]).shape[0]
    assert info["batch"] + info["tie"] + info["emulated"] == n_uniq     # each unique source in one tier
    if name == "dense":
        assert eng.stats()["mode"] == 3
    eng.close()


@pytest.mark.parametrize("name", ["tiefree_batched", "quantized_batched", "directed_batched",
                                  "powerlaw_batched"])
def test_tiers_agree(E, name, monkeypatch):
    """Batched mode: the batch tier (walks over the split kernels' persisted
    distances), the tie tier (walks over the early-stop tie rows' final
    parents) and the grouped emulation alone give the same bytes."""
    top, att, force, _ = _case(name)
    src, dst = _requests(att, n_src=att.shape[0], n_dst=3)    # every row: the tie rows are among them
    n_uniq = np.unique(src[src != dst]).shape[0]
    eng = E.Engine(top, att, force_mode=force)
    assert eng.stats()["batched"] == 1
    fast = eng.get_paths(src, dst, hops=True)
    info = eng.paths_info()
    eng.close()
    print(name, info)
    assert info["batch"] > 0
    if name == "tiefree_batched":
        assert info["emulated"] == 0 and info["groups"] == 0 and info["handed_on"] == 0
        assert info["batch"] == n_uniq and info["tie"] == 0
    if name == "quantized_batched":
        assert info["tie"] > 0                            # its tie rows, served from their tie slots
    assert info["batch"] + info["tie"] + info["emulated"] == n_uniq
    monkeypatch.setenv("SHDPE_PATHS_FAST", "0")
    eng = E.Engine(top, att, force_mode=force, debug_flags=E.DEBUG_ENV)
    slow = eng.get_paths(src, dst, hops=True)
    info = eng.paths_info()
    eng.close()
    assert info["batch"] == 0 and info["tie"] == 0 and info["emulated"] == n_uniq
    for f, s in zip(fast, slow):
        assert f.tobytes() == s.tobytes()


@pytest.mark.parametrize("corrupt", [1, 2])
def test_bad_tie_slot_is_handed_on(E, corrupt, monkeypatch):
    """A tie slot holding distances that are not its row's (SHDPE_TIE_CORRUPT:
    halved, or shifted off the source) fails the early-stop emulation's
    consistency check or the walk's arrival check: the tie tier hands the row's
    requests on and the grouped emulation gives the same bytes."""
    top, att, force, _ = _case("quantized_batched")
    src, dst = _requests(att, n_src=att.shape[0], n_dst=3)
    eng = E.Engine(top, att, force_mode=force)
    ref = eng.get_paths(src, dst, hops=True)
    ref_info = eng.paths_info()
    ck = eng.row_checksums(0, eng.T)
    eng.close()
    assert ref_info["tie"] > 0 and ref_info["handed_on"] == 0 and ref_info["emulated"] == 0
    monkeypatch.setenv("SHDPE_TIE_CORRUPT", str(corrupt))
    eng = E.Engine(top, att, force_mode=force, debug_flags=E.DEBUG_ENV)
    got = eng.get_paths(src, dst, hops=True)
    info = eng.paths_info()
    print(corrupt, info)
    assert info["handed_on"] > 0 and info["emulated"] > 0 and info["groups"] > 0
    assert info["tie"] < ref_info["tie"]
    assert info["batch"] + info["tie"] + info["emulated"] == ref_info["batch"] + ref_info["tie"]
    for g, r in zip(got, ref):
        assert g.tobytes() == r.tobytes()
    assert np.array_equal(eng.row_checksums(0, eng.T), ck)
    eng.close()


def test_partial_hand_on_counts_once(E, monkeypatch):
    """A corrupted tie slot sends its row's requests through every tier: each
    unique source is still counted once, the sources of the untouched tiers
    keep their counter, and the bytes are those of the uncorrupted run."""
    top, att, force, _ = _case("quantized_batched")
    src, dst = _requests(att, n_src=att.shape[0], n_dst=3)
    for s in np.unique(src):                              # (CPU) several targets per source
        assert np.unique(dst[src == s]).shape[0] >= 2, s
    n_uniq = np.unique(src[src != dst]).shape[0]
    eng = E.Engine(top, att, force_mode=force)
    ref = eng.get_paths(src, dst, hops=True)
    ref_info = eng.paths_info()
    eng.close()
    monkeypatch.setenv("SHDPE_TIE_CORRUPT", "2")
    eng = E.Engine(top, att, force_mode=force, debug_flags=E.DEBUG_ENV)
    got = eng.get_paths(src, dst, hops=True)
    info = eng.paths_info()
    eng.close()
    print(ref_info, info)
    assert ref_info["batch"] + ref_info["tie"] + ref_info["emulated"] == n_uniq
    assert info["batch"] + info["tie"] + info["emulated"] == n_uniq
    # a source under `emulated` is in no other counter: the batch tier's sources
    # are the same in both runs, and what the tie tier lost the emulation gained
    assert info["emulated"] > ref_info["emulated"] and info["handed_on"] > 0
    assert info["batch"] == ref_info["batch"]
    assert info["emulated"] - ref_info["emulated"] == ref_info["tie"] - info["tie"]
    for g, r in zip(got, ref):
        assert g.tobytes() == r.tobytes()


def test_grouping_and_chunking(E, oracle_mod, monkeypatch):
    """600 unique sources in emulation groups of 64 and staging chunks of 100
    requests: the same bytes as the unchunked call."""
    top = G.random_sparse(800, 5, seed=34)
    att = np.arange(800, dtype=np.int32)
    rng = np.random.default_rng(9)
    src = rng.permutation(att)[:600].astype(np.int32)
    dst = rng.choice(att, 600).astype(np.int32)
    eng = E.Engine(top, att)
    ref = eng.get_paths(src, dst, hops=True)
    ref_info = eng.paths_info()
    eng.close()
    monkeypatch.setenv("SHDPE_PATHS_GROUP", "64")
    monkeypatch.setenv("SHDPE_PATHS_CHUNK", "100")
    eng = E.Engine(top, att, debug_flags=E.DEBUG_ENV)
    got = eng.get_paths(src, dst, hops=True)
    info = eng.paths_info()
    eng.close()
    for g, r in zip(got, ref):
        assert g.tobytes() == r.tobytes()
    assert info["groups"] >= 10 and info["groups"] > ref_info["groups"]
    assert info["emulated"] == 600
    orc = _Oracle(oracle_mod, top, att)
    offsets, verts = got[0], got[1]
    for i in range(0, 600, 7):
        assert verts[offsets[i]:offsets[i + 1]].tolist() == orc.path(src[i], dst[i])


def test_equals_loop_of_get_path(E):
    """60 mixed requests (reachable, src == dst, unattached, out of range,
    repeated): path and code of shd_pe_get_path, one by one."""
    top = G.random_sparse(500, 5, seed=36, quantum=1.0)
    att = np.arange(0, 500, 2, dtype=np.int32)
    rng = np.random.default_rng(3)
    src = rng.choice(att, 60).astype(np.int32)
    dst = rng.choice(att, 60).astype(np.int32)
    dst[::6] = src[::6]
    src[5], dst[11], src[17], dst[23] = 1, 3, -1, 500      # unattached, out of range
    src[40:44], dst[40:44] = src[30:34], dst[30:34]
    eng = E.Engine(top, att)
    offsets, verts, status = eng.get_paths(src, dst)
    for i in range(60):
        try:
            exp, code = eng.get_path(int(src[i]), int(dst[i])), 0
        except E.EngineError as e:
            exp, code = [], e.code
        assert status[i] == code, (i, src[i], dst[i])
        assert verts[offsets[i]:offsets[i + 1]].tolist() == exp, (i, src[i], dst[i])
    assert set(status.tolist()) >= {0, E.ENOTATTACHED, E.EINVAL}
    # the one-pair call's cached parent array does not survive the batched call
    s, t = int(att[3]), int(att[100])
    one = eng.get_path(s, t)
    eng.get_paths(src, dst)
    assert eng.get_path(s, int(att[7])) == eng.get_paths([s], [int(att[7])])[1].tolist()
    assert eng.get_path(s, t) == one
    eng.close()


@pytest.mark.parametrize("force_mode", [0, 5])
def test_get_path_cap_boundary(E, force_mode):
    """shd_pe_get_path with a capacity of exactly the path's length returns the
    path; one short is SHD_PE_EINVAL, and the refusal leaves the cached source
    usable.  (force_mode 5 relabels the vertices on the device.)"""
    top = G.random_sparse(500, 5, seed=36, quantum=1.0)
    att = np.arange(0, 500, 2, dtype=np.int32)
    rng = np.random.default_rng(11)
    src = np.repeat(rng.choice(att, 3, replace=False), 20).astype(np.int32)
    dst = rng.choice(att, src.shape[0]).astype(np.int32)
    eng = E.Engine(top, att, force_mode=force_mode)
    offsets, verts, status = eng.get_paths(src, dst)
    lens = np.diff(offsets)
    picks = [i for i in range(src.shape[0]) if status[i] == 0 and lens[i] >= 3][:5]
    assert len(picks) == 5                                # (of the first source or two: the cached walk)
    for i in picks:
        s, t, n = int(src[i]), int(dst[i]), int(lens[i])
        want = verts[offsets[i]:offsets[i + 1]].tolist()
        assert eng.get_path(s, t, cap=n) == want, (s, t)
        with pytest.raises(E.EngineError) as err:
            eng.get_path(s, t, cap=n - 1)
        assert err.value.code == E.EINVAL, (s, t)
        assert eng.get_path(s, t) == want, (s, t)
    eng.close()


@pytest.mark.parametrize("force_mode", [0, 5])
def test_get_path_many_targets_one_emulation(E, force_mode):
    """One shd_pe_get_path per attached target of a source (the cached parent
    array walked hundreds of times): path and code of shd_pe_get_paths for the
    same pairs (SHD_PE_EUNREACHABLE in both where the directed graph has no path)."""
    top = G.random_sparse(700, 5, seed=31, directed=True)
    att = np.arange(0, 700, 3, dtype=np.int32)
    eng = E.Engine(top, att, force_mode=force_mode)
    srcs = att[[1, 60, 117, 230]]
    src = np.repeat(srcs, att.shape[0]).astype(np.int32)
    dst = np.tile(att, srcs.shape[0]).astype(np.int32)
    offsets, verts, status = eng.get_paths(src, dst)
    assert set(status.tolist()) <= {0, E.EUNREACHABLE} and np.count_nonzero(status == 0) > 800
    for i in range(src.shape[0]):
        try:
            one, code = eng.get_path(int(src[i]), int(dst[i])), 0
        except E.EngineError as e:
            one, code = [], e.code
        assert code == status[i], (i, src[i], dst[i])
        assert one == verts[offsets[i]:offsets[i + 1]].tolist(), (i, src[i], dst[i])
    eng.close()


@pytest.mark.parametrize("force_mode", [0, 5])
def test_failures_are_per_request(E, oracle_mod, force_mode):
    """Two disjoint components: unreachable pairs are SHD_PE_EUNREACHABLE with
    an empty path, their neighbours in the same call are right."""
    a, b = G.random_sparse(300, 4, seed=41), G.random_sparse(200, 4, seed=42)
    top = Topology(n=500, directed=False, src=np.concatenate([a.src, b.src + 300]),
                   dst=np.concatenate([a.dst, b.dst + 300]),
                   latency=np.concatenate([a.latency, b.latency]),
                   loss=np.concatenate([a.loss, b.loss]))
    att = np.arange(0, 500, 5, dtype=np.int32)
    eng = E.Engine(top, att, force_mode=force_mode)
    orc = _Oracle(oracle_mod, top, att)
    src = np.array([10, 0, 10, 310, 305, 5, 450, 10, 1, 10, 500, -1, 20], np.int32)
    dst = np.array([20, 305, 295, 5, 400, 400, 10, 20, 10, 2, 10, 10, 20], np.int32)
    want = [0, E.EUNREACHABLE, 0, E.EUNREACHABLE, 0, E.EUNREACHABLE, E.EUNREACHABLE, 0,
            E.ENOTATTACHED, E.ENOTATTACHED, E.EINVAL, E.EINVAL, 0]
    offsets, verts, status, hl, hr = eng.get_paths(src, dst, hops=True)
    assert status.tolist() == want
    for i, w in enumerate(want):
        p = verts[offsets[i]:offsets[i + 1]].tolist()
        assert p == ([] if w else orc.path(src[i], dst[i])), i
    assert offsets[-1] == verts.shape[0] == hl.shape[0] == hr.shape[0]
    eng.close()


def test_complete_graph_and_missing_self_loop(E, oracle_mod):
    top = Topology.load_npz(os.path.join(GOLDEN, "shipped_topology.npz"), name="shipped")
    att = np.arange(0, top.n, 2, dtype=np.int32)
    eng = E.Engine(top, att)
    assert eng.is_complete
    og = oracle_mod.OracleGraph(top)
    src, dst = _requests(att, n_src=12, n_dst=4)
    offsets, verts, status, hl, hr = eng.get_paths(src, dst, hops=True)
    assert not status.any()
    for i in range(src.shape[0]):
        p = verts[offsets[i]:offsets[i + 1]].tolist()
        assert p == ([int(src[i])] if src[i] == dst[i] else [int(src[i]), int(dst[i])])
        assert p == eng.get_path(int(src[i]), int(dst[i]))
        if len(p) == 2:
            e = og.get_eid(p[0], p[1])
            assert _bits([hl[offsets[i] + 1]])[0] == _bits([top.latency[e]])[0]
            assert _bits([hr[offsets[i] + 1]])[0] == _bits([1.0 - top.loss[e]])[0]
    assert eng.paths_info()["groups"] == 0
    eng.close()
    # src == dst on a vertex without a self-loop: the table entry is F_NOEDGE, the path is [s]
    top = G.random_sparse(200, 4, seed=7, self_loops=False)
    att = np.arange(0, 200, 2, dtype=np.int32)
    eng = E.Engine(top, att)
    assert eng.get_row(4)["flags"][2] & E.F_NOEDGE
    offsets, verts, status = eng.get_paths([4, 4, 6], [4, 6, 6])
    assert status.tolist() == [0, 0, 0]
    assert verts[:1].tolist() == [4] and verts[offsets[2]:].tolist() == [6]
    assert verts[offsets[1]:offsets[2]].tolist() == eng.get_path(4, 6)
    eng.close()


def test_sizing_protocol(E):
    """verts == NULL fills offsets and status without an emulation; a capacity
    one short is SHD_PE_EINVAL with the offsets intact."""
    top = G.random_sparse(400, 5, seed=37)
    att = np.arange(0, 400, 2, dtype=np.int32)
    eng = E.Engine(top, att)
    src, dst = _requests(att, n_src=10, n_dst=5)
    n = src.shape[0]
    ref_off, ref_verts, ref_status = eng.get_paths(src, dst)
    lib = E.load_library()

    def call(verts, cap):
        offsets = np.full(n + 1, -1, np.int64)
        status = np.full(n, 99, np.int32)
        o = E.PathsOutC(offsets.ctypes.data_as(C.c_void_p),
                        None if verts is None else verts.ctypes.data_as(C.c_void_p), None, None,
                        status.ctypes.data_as(C.c_void_p), cap)
        rc = lib.shd_pe_get_paths(eng.h, src.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p),
                                  n, C.byref(o))
        return rc, offsets, status

    rc, offsets, status = call(None, 0)
    assert rc == 0 and np.array_equal(offsets, ref_off) and np.array_equal(status, ref_status)
    info = eng.paths_info()
    assert info["groups"] == 0 and info["emulated"] == 0 and info["batch"] == 0 and info["tie"] == 0
    total = int(ref_off[-1])
    verts = np.full(total, -5, np.int32)
    rc, offsets, status = call(verts, total - 1)
    assert rc == E.EINVAL and np.array_equal(offsets, ref_off) and np.array_equal(status, ref_status)
    assert np.all(verts == -5) and eng.paths_info()["groups"] == 0
    rc, offsets, status = call(verts, total)
    assert rc == 0 and np.array_equal(verts, ref_verts)
    # an empty call
    o = E.PathsOutC(offsets.ctypes.data_as(C.c_void_p), None, None, None, None, 0)
    assert lib.shd_pe_get_paths(eng.h, None, None, 0, C.byref(o)) == 0 and offsets[0] == 0
    eng.close()


def test_sharding(E, oracle_mod):
    """Two logical shards on one device give the bytes of one shard; an
    ungathered engine of a two-engine split answers SHD_PE_ENOTOWNED per
    request for the other engine's sources."""
    top = G.random_sparse(800, 5, seed=32, quantum=0.5)
    att = np.arange(0, 800, 2, dtype=np.int32)
    src, dst = _requests(att, n_src=60, n_dst=4, seed=8)
    eng = E.Engine(top, att, force_mode=5)
    ref = eng.get_paths(src, dst, hops=True)
    eng.close()
    eng = E.Engine(top, att, force_mode=5, devices=[0, 0])
    got = eng.get_paths(src, dst, hops=True)
    bounds = eng.shard_bounds()
    eng.close()
    for g, r in zip(got, ref):
        assert g.tobytes() == r.tobytes()
    pos = {int(v): k for k, v in enumerate(att)}
    sides = {int(pos[int(s)] >= bounds[1]) for s in src}
    assert sides == {0, 1}                                # both shards served requests
    eng = E.Engine(top, att, force_mode=5, shard_index=0, shard_count=2)
    lo, cnt = eng.owned
    offsets, verts, status = eng.get_paths(src, dst)
    foreign = 0
    for i in range(src.shape[0]):
        p = verts[offsets[i]:offsets[i + 1]].tolist()
        own = lo <= pos[int(src[i])] < lo + cnt
        if src[i] == dst[i] or own:
            assert status[i] == 0 and p == ref[1][ref[0][i]:ref[0][i + 1]].tolist(), i
        else:
            assert status[i] == E.ENOTOWNED and p == [], i
            foreign += 1
        try:                                              # the one-pair call on the same engine
            one, code = eng.get_path(int(src[i]), int(dst[i])), 0
        except E.EngineError as e:
            one, code = [], e.code
        assert (code, one) == (int(status[i]), p), i
    assert foreign > 0
    eng.close()


@pytest.mark.parametrize("quantum,force_mode", [(0.0, 0), (0.0, 5), (0.5, 5)])
def test_no_side_effects(E, quantum, force_mode):
    """The rows the emulation rewrites keep their bytes (flags included: the
    tie-free graph's rows all came from the fast path, without F_EXACT), and
    neither the counters of ShdPeStats nor the computed-row state move."""
    top = G.random_sparse(800, 5, seed=34 if quantum == 0.0 else 32, quantum=quantum)
    att = np.arange(0, 800, 3, dtype=np.int32)
    eng = E.Engine(top, att, force_mode=force_mode)
    eng.compute_all()
    T = eng.T
    before, ck = eng.stats(), eng.row_checksums(0, T)
    rows = eng.get_rows(0, T)
    assert (before["rowsExact"] == 0) == (quantum == 0.0)
    src, dst = _requests(att, n_src=80, n_dst=3, seed=6)
    eng.get_paths(src, dst, hops=True)
    assert eng.paths_info()["emulated"] + eng.paths_info()["batch"] + eng.paths_info()["tie"] > 0
    assert eng.stats() == before
    assert np.array_equal(eng.row_checksums(0, T), ck)
    after = eng.get_rows(0, T)
    for k, v in rows.items():
        assert v.tobytes() == after[k].tobytes(), k
    eng.close()
    # rows not computed yet are computed first, as in get_rows
    eng = E.Engine(top, att, force_mode=force_mode)
    offsets, verts, status = eng.get_paths(src[:9], dst[:9])
    assert eng.stats()["rowsComputed"] == np.unique(src[:9][src[:9] != dst[:9]]).shape[0]
    assert not status.any()
    eng.close()
