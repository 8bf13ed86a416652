"""GPU tests of the link / vertex load reduction (shd_pe_path_load, the arc
list, shd_topology_link_load): the sums against numpy over the paths
shd_pe_get_paths returns for the same requests, and over the oracle's igraph
paths; in every mode and tier, with failures, 64-bit weights, any request
order and chunking, two shards, no side effects, and the mirror's teardown
call against its own cache."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from shdpe import generators as G
from shdpe.graph import Topology
from test_gpu_paths import CASES, E, _Oracle, _requests  # noqa: F401  (E: the fixture)

pytestmark = pytest.mark.gpu

U64 = np.uint64
COMPLETE = "complete"
TIERS = ("batch", "tie", "emulated", "rows")


def _shipped():
    return Topology.load_npz(os.path.join(GOLDEN, "shipped_topology.npz"), name="shipped")


def _engine(E, name, row_tier=False, **kw):
    if name == COMPLETE:
        top, force = _shipped(), 0
    else:
        make, _, force, _ = CASES[name]
        top = make()
    att = np.arange(0, top.n, 3, dtype=np.int32)
    eng = E.Engine(top, att, force_mode=force, **kw)
    if row_tier:
        eng.set_paths_row_tier(True)
    return eng, att


def _weights(n, seed=7):
    """Random weights in [0, 2^40], weight 0 among them."""
    w = np.random.default_rng(seed).integers(0, 2 ** 40, n, endpoint=True).astype(U64)
    w[::11] = 0
    return w


def _arc_index(eng):
    af, at = eng.arcs()
    return af.astype(np.int64) * eng.top.n + at


def _sum_paths(eng, offsets, verts, w):
    """arc / vertex sums (uint64, mod 2^64) of weighted paths given as get_paths gives them."""
    key = _arc_index(eng)
    n = eng.top.n
    lens = np.diff(offsets)
    wi = np.repeat(np.asarray(w, U64), lens)
    verts = np.asarray(verts, np.int64)
    vertex = np.zeros(n, U64)
    np.add.at(vertex, verts, wi)
    first = np.zeros(verts.shape[0], bool)
    first[offsets[:-1][lens > 0]] = True
    hop = np.flatnonzero(~first)
    k = verts[hop - 1] * n + verts[hop]
    a = np.searchsorted(key, k)
    assert np.array_equal(key[a], k)                      # every hop is an arc
    arc = np.zeros(key.shape[0], U64)
    np.add.at(arc, a, wi[hop])
    return arc, vertex


def _expected(eng, src, dst, w):
    offsets, verts, status = eng.get_paths(src, dst)
    arc, vertex = _sum_paths(eng, offsets, verts, w)
    return {"arc": arc, "vertex": vertex, "status": status, "lens": np.diff(offsets)}


def _same(got, exp):
    assert np.array_equal(got["arc"], exp["arc"])
    assert np.array_equal(got["vertex"], exp["vertex"])
    if "status" in exp and "status" in got:
        assert np.array_equal(got["status"], exp["status"])


def _usum(a):
    return int(np.sum(np.asarray(a, U64), dtype=U64))


def _n_uniq(src, dst, status):
    return np.unique(src[(src != dst) & (status == 0)]).shape[0]


# ---- 1. every mode --------------------------------------------------------------

MODES = [("tiefree", False), ("tiefree_batched", False), ("quantized_batched", False),
         ("directed_batched", False), ("powerlaw_batched", False), ("vloss", False), ("latfold", False),
         ("dense", False), ("dense", True), (COMPLETE, False)]


@pytest.mark.parametrize("name,row_tier", MODES, ids=[n + ("_rows" if r else "") for n, r in MODES])
def test_every_mode(E, name, row_tier):
    eng, att = _engine(E, name, row_tier)
    src, dst = _requests(att, n_src=att.shape[0], n_dst=3)
    w = _weights(src.shape[0])
    assert np.any(src == dst) and np.any(w == 0)
    exp = _expected(eng, src, dst, w)
    assert int(exp["lens"].sum()) % 256 != 0
    got = eng.path_load(src, dst, w)
    info = eng.paths_info()
    print(name, row_tier, info, got["totals"])
    _same(got, exp)
    assert int(got["totals"][0]) == np.count_nonzero(exp["status"] == 0)
    assert int(got["totals"][3]) == np.count_nonzero(exp["status"])
    assert int(got["totals"][1]) == _usum(got["vertex"])
    assert int(got["totals"][2]) == _usum(got["arc"])
    # ... and the table's hops alone give the same two sums
    pos = {int(v): k for k, v in enumerate(eng.attached)}
    hops = np.zeros(src.shape[0], U64)
    rows = {}
    for i in range(src.shape[0]):
        s, t = int(src[i]), int(dst[i])
        if s == t or exp["status"][i]:
            continue
        if s not in rows:
            rows[s] = eng.get_row(s)["hops"]
        hops[i] = rows[s][pos[t]]
    ok = (exp["status"] == 0).astype(U64)
    assert int(got["totals"][2]) == _usum(w * hops * ok)
    assert int(got["totals"][1]) == _usum(w * (hops + U64(1)) * ok)
    n_uniq = 0 if name == COMPLETE else _n_uniq(src, dst, exp["status"])
    assert sum(info[k] for k in TIERS) == n_uniq          # each unique source in exactly one tier
    if row_tier:
        assert info["rows"] > 0
    if name.endswith("_batched"):
        assert info["batch"] > 0
    if name == "quantized_batched":
        assert info["tie"] > 0
    eng.close()


# ---- 2. against the oracle directly ---------------------------------------------

@pytest.mark.parametrize("name", ["tiefree", "quantized"])
def test_against_oracle(E, oracle_mod, name):
    eng, att = _engine(E, name)
    orc = _Oracle(oracle_mod, eng.top, eng.attached)
    src, dst = _requests(att, n_src=60, n_dst=4)
    w = _weights(src.shape[0], seed=8)
    paths = [orc.path(s, t) for s, t in zip(src, dst)]
    assert all(p is not None for p in paths)
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
    arc, vertex = _sum_paths(eng, offsets, np.concatenate(paths), w)
    got = eng.path_load(src, dst, w)
    assert not got["status"].any()
    _same(got, {"arc": arc, "vertex": vertex})
    eng.close()


# ---- 3. the arc list ------------------------------------------------------------

def test_arc_list(E):
    top = G.with_parallel_loops(G.random_sparse(300, 5, seed=12), 0.5, seed=3)
    att = np.arange(0, 300, 2, dtype=np.int32)
    eng = E.Engine(top, att)
    af, at = eng.arcs()
    assert af.shape[0] == eng.stats()["nArcs"] == at.shape[0]
    key = af.astype(np.int64) * top.n + at
    assert np.all(np.diff(key) > 0)                       # sorted by (from, to), no duplicates
    assert not np.any(af == at)
    edges = {(int(a), int(b)) for a, b in zip(top.src, top.dst) if a != b}
    edges |= {(b, a) for a, b in edges}
    assert edges == set(zip(af.tolist(), at.tolist()))
    rng = np.random.default_rng(4)
    pairs = list(zip(rng.integers(0, 300, 100).tolist(), rng.integers(0, 300, 100).tolist()))
    pairs += [(int(af[k]), int(at[k])) for k in rng.integers(0, af.shape[0], 100)]
    for s, t in pairs:
        if s == t:
            continue
        hit = np.flatnonzero(key == s * top.n + t)
        assert eng.find_arc(s, t) == (int(hit[0]) if hit.shape[0] else -1), (s, t)
    non_edge = next((s, t) for s in range(300) for t in range(300) if s != t and (s, t) not in edges)
    assert eng.find_arc(*non_edge) == -1
    loop = int(top.src[top.src == top.dst][0])
    assert eng.find_arc(loop, loop) == -2
    assert eng.find_arc(-1, 0) == -1 and eng.find_arc(0, 300) == -1
    eng.close()


# ---- 4. failures add nothing ----------------------------------------------------

def test_failures_add_nothing(E):
    base = G.random_sparse(700, 5, seed=31, directed=True)
    # vertex 700 has an out-arc only: no source reaches it
    top = Topology(n=701, directed=True, src=np.concatenate([base.src, [700]]),
                   dst=np.concatenate([base.dst, [0]]), latency=np.concatenate([base.latency, [3.0]]),
                   loss=np.concatenate([base.loss, [0.0]]))
    att = np.concatenate([np.arange(0, 700, 3), [700]]).astype(np.int32)
    eng = E.Engine(top, att)
    src, dst = _requests(att[:-1], n_src=50, n_dst=3)
    # out of range (3), unattached source / target, unreachable (2), and the path [700]
    bad_s = np.array([-1, 701, 1, 3, 6, 9, 700, 12], np.int32)
    bad_d = np.array([3, 3, 3, 2, 700, 700, 700, 9000], np.int32)
    mix = np.random.default_rng(14).permutation(src.shape[0] + bad_s.shape[0])
    asrc, adst = np.concatenate([src, bad_s])[mix], np.concatenate([dst, bad_d])[mix]
    w = _weights(asrc.shape[0], seed=9) + U64(1)
    ref = eng.get_paths(asrc, adst)[2]
    assert set(ref.tolist()) == {0, E.EINVAL, E.ENOTATTACHED, E.EUNREACHABLE}
    good = ref == 0
    assert np.count_nonzero(~good) == 7                   # (700 -> 700 is the path [700])
    got = eng.path_load(asrc, adst, w)
    assert np.array_equal(got["status"], ref)
    assert int(got["totals"][3]) == 7 and int(got["totals"][0]) == asrc.shape[0] - 7
    alone = eng.path_load(asrc[good], adst[good], w[good])
    assert not alone["status"].any() and int(alone["totals"][3]) == 0
    _same({k: got[k] for k in ("arc", "vertex")}, {k: alone[k] for k in ("arc", "vertex")})
    _same(alone, _expected(eng, asrc[good], adst[good], w[good]))
    assert np.array_equal(got["totals"][1:3], alone["totals"][1:3])
    # nothing but failures: every sum is zero
    none = eng.path_load(asrc[~good], adst[~good], w[~good])
    assert not none["arc"].any() and not none["vertex"].any() and none["totals"].tolist() == [0, 0, 0, 7]
    eng.close()


# ---- 5. 64-bit sums -------------------------------------------------------------

def test_64_bit_sums(E):
    eng, att = _engine(E, "tiefree")
    s, t = int(att[5]), int(att[150])
    path = eng.get_path(s, t)
    assert len(path) >= 3
    got = eng.path_load([s, s], [t, t], np.array([2 ** 63, 2 ** 63], U64))
    assert not got["arc"].any() and not got["vertex"].any()
    assert got["totals"].tolist() == [2, 0, 0, 0]
    big = U64(2 ** 33)
    got = eng.path_load([s, s, s], [t, t, s], np.array([big, 5, 1], U64))
    assert got["vertex"][path[1]] == big + U64(5) and got["vertex"][s] == big + U64(6)
    a = eng.find_arc(path[0], path[1])
    assert a >= 0 and got["arc"][a] == big + U64(5)
    assert int(got["arc"].sum(dtype=U64)) == (2 ** 33 + 5) * (len(path) - 1)
    src, dst = _requests(att, n_src=40, n_dst=3)
    ones = eng.path_load(src, dst, np.ones(src.shape[0], U64))
    none = eng.path_load(src, dst)
    _same(none, ones)
    assert np.array_equal(none["totals"], ones["totals"])
    _same(none, _expected(eng, src, dst, np.ones(src.shape[0], U64)))
    # an empty call overwrites with zeros
    empty = eng.path_load([], [])
    assert not empty["arc"].any() and not empty["vertex"].any() and not empty["totals"].any()
    eng.close()


# ---- 6. order and chunks --------------------------------------------------------

def test_order_and_chunks(E, monkeypatch):
    eng, att = _engine(E, "tiefree_batched")
    src, dst = _requests(att, n_src=att.shape[0], n_dst=3)
    w = _weights(src.shape[0], seed=10)
    ref = eng.path_load(src, dst, w)
    _same(ref, _expected(eng, src, dst, w))
    perm = np.random.default_rng(11).permutation(src.shape[0])
    shuf = eng.path_load(src[perm], dst[perm], w[perm])
    _same({k: shuf[k] for k in ("arc", "vertex")}, {k: ref[k] for k in ("arc", "vertex")})
    assert np.array_equal(shuf["status"], ref["status"][perm])
    assert np.array_equal(shuf["totals"], ref["totals"])
    eng.close()
    monkeypatch.setenv("SHDPE_PATHS_CHUNK", "100")
    monkeypatch.setenv("SHDPE_PATHS_GROUP", "7")
    eng, _ = _engine(E, "tiefree_batched", debug_flags=E.DEBUG_ENV)
    got = eng.path_load(src[perm], dst[perm], w[perm])
    info = eng.paths_info()
    _same(got, shuf)
    assert np.array_equal(got["totals"], ref["totals"])
    n_uniq = _n_uniq(src, dst, ref["status"])
    passes = sum(info[k] for k in TIERS)
    print(info, n_uniq, src.shape[0])
    # the requests are sorted by source: a source is served again only where its
    # requests straddle a chunk boundary
    assert n_uniq <= passes <= n_uniq + -(-src.shape[0] // 100)
    eng.close()
    # without the sort the shuffled list pays a pass per source per chunk
    monkeypatch.setenv("SHDPE_LOAD_SORT", "0")
    eng, _ = _engine(E, "tiefree_batched", debug_flags=E.DEBUG_ENV)
    unsorted = eng.path_load(src[perm], dst[perm], w[perm])
    info = eng.paths_info()
    _same(unsorted, shuf)
    assert sum(info[k] for k in TIERS) > n_uniq + -(-src.shape[0] // 100)
    eng.close()


# ---- 7. two logical shards ------------------------------------------------------

@pytest.mark.parametrize("name", ["tiefree", "quantized_batched"])
def test_two_shards(E, name):
    eng, att = _engine(E, name)
    src, dst = _requests(att, n_src=att.shape[0], n_dst=3)
    w = _weights(src.shape[0], seed=12)
    ref = eng.path_load(src, dst, w)
    eng.close()
    eng, _ = _engine(E, name, devices=[0, 0])
    got = eng.path_load(src, dst, w)
    bounds = eng.shard_bounds()
    eng.close()
    assert len(bounds) == 3 and 0 < bounds[1] < att.shape[0]
    _same(got, ref)
    assert np.array_equal(got["totals"], ref["totals"])


# ---- 8. no side effects ---------------------------------------------------------

def test_no_side_effects(E):
    eng, att = _engine(E, "quantized_batched")
    eng.compute_all()
    T = eng.T
    s, t = int(att[3]), int(att[50])
    one = eng.get_path(s, t)
    before, ck = eng.stats(), eng.row_checksums(0, T)
    picks = [int(att[0]), s, int(att[-1])]
    rows = [eng.get_row(v) for v in picks]
    src, dst = _requests(att, n_src=att.shape[0], n_dst=3)
    eng.path_load(src, dst, _weights(src.shape[0]))
    info = eng.paths_info()
    assert info["batch"] > 0 and info["tie"] + info["emulated"] > 0
    assert eng.stats() == before
    assert np.array_equal(eng.row_checksums(0, T), ck)
    for v, row in zip(picks, rows):
        after = eng.get_row(v)
        for key, val in row.items():
            assert val.tobytes() == after[key].tobytes(), (v, key)
    assert eng.get_path(s, t) == one
    eng.close()
    # rows not computed yet are computed first
    eng, _ = _engine(E, "quantized_batched")
    got = eng.path_load(src[:9], dst[:9])
    assert not got["status"].any()
    assert eng.stats()["rowsComputed"] == np.unique(src[:9][src[:9] != dst[:9]]).shape[0]
    eng.close()


# ---- 9. the reduction's LDS table ------------------------------------------------

def test_lds_table_and_overflow(E, monkeypatch):
    """Contended hub arcs: the workgroup's LDS table combines adds before they
    are issued; with a table of 8 slots most adds overflow their probes into
    the global fallback.  The sums are the same."""
    atomics = {}
    for slots in (None, "8"):
        if slots:
            monkeypatch.setenv("SHDPE_LOAD_SLOTS", slots)
        eng, att = _engine(E, "powerlaw_batched", debug_flags=E.DEBUG_ENV | E.DEBUG_COUNTERS)
        src, dst = _requests(att, n_src=att.shape[0], n_dst=3)
        w = _weights(src.shape[0], seed=15)
        exp = _expected(eng, src, dst, w)
        got = eng.path_load(src, dst, w)
        li = eng.path_load_info()
        eng.close()
        _same(got, exp)
        assert li["entries"] == int(exp["lens"].sum())
        atomics[slots] = li["atomics"]
    # one add per entry's vertex and per hop where nothing is combined (weight 0 adds nothing);
    # a slot is flushed with one add for at least one combined, so never more than that
    lens = exp["lens"]
    uncombined = int(np.sum((2 * lens - 1)[(lens > 0) & (w != 0)]))
    print(atomics, uncombined)
    assert 0 < atomics[None] < atomics["8"] <= uncombined


# ---- 10. the mirror's teardown call ---------------------------------------------

def _mirror_pairs(top, att, rng):
    adj = [(int(a), int(b)) for a, b in zip(top.src, top.dst) if a != b and a % 3 == 0 and b % 3 == 0]
    pairs = [(int(a), int(b)) for a, b in zip(rng.choice(att, 230), rng.choice(att, 230))]
    pairs += [(int(v), int(v)) for v in rng.choice(att, 10)]
    pairs += adj[:30]
    far = [(int(att[2]), int(att[-3])), (int(att[-3]), int(att[2]))] * 8       # one pair, both directions
    pairs += far + pairs[:14]                                                # ... and repeats
    return [pairs[k] for k in rng.permutation(len(pairs))]


@pytest.mark.parametrize("name", ["sparse", COMPLETE])
def test_mirror_link_load(E, name):
    top = _shipped() if name == COMPLETE else G.random_sparse(800, 5, seed=34)
    att = np.arange(0, top.n, 3, dtype=np.int32)
    eng = E.Engine(top, att)
    shim = E.TopologyShim(eng, prefers_direct=True)
    empty = shim.link_load()
    assert not empty["arc"].any() and not empty["vertex"].any() and not empty["totals"].any()
    pairs = _mirror_pairs(top, att, np.random.default_rng(13))
    assert 280 <= len(pairs) <= 320
    for s, d in pairs:
        assert shim.increment(s, d) == 0
    n = top.n
    arc, vertex = np.zeros(eng.arcs()[0].shape[0], U64), np.zeros(n, U64)
    req, hops_sum, packets, kinds = [], 0, 0, set()
    for s, d in sorted({(min(p), max(p)) for p in pairs}):
        for a, b in ((s, d), (d, s)) if s != d else ((s, d),):
            c = shim.cached(a, b)
            if c is None:
                continue
            _, _, direct, pc = c
            assert pc > 0
            packets += pc
            if a == b:
                vertex[a] += U64(pc)
                kinds.add("self")
            elif direct:
                vertex[a] += U64(pc)
                vertex[b] += U64(pc)
                k = eng.find_arc(a, b)
                assert k >= 0
                arc[k] += U64(pc)
                hops_sum += pc
                kinds.add("direct")
            else:
                req.append((a, b, pc))
                kinds.add("path")
    assert packets == len(pairs)                          # every increment landed in one stored entry
    assert kinds == ({"self", "direct"} if name == COMPLETE else {"self", "direct", "path"})
    if req:
        rs, rd, rw = (np.array(x) for x in zip(*req))
        offsets, verts, status = eng.get_paths(rs, rd)
        assert not status.any()
        a2, v2 = _sum_paths(eng, offsets, verts, rw.astype(U64))
        arc += a2
        vertex += v2
        hops_sum += int(np.sum((np.diff(offsets) - 1) * rw))
    got = shim.link_load()
    _same(got, {"arc": arc, "vertex": vertex})
    assert int(got["totals"][2]) == hops_sum % 2 ** 64 == _usum(got["arc"])
    assert int(got["totals"][1]) == _usum(got["vertex"])
    assert int(got["totals"][3]) == 0
    # a counter of 2^33 + 1 packets, by weight (increment adds one at a time)
    if req:
        s, d, _ = req[0]
        big = 2 ** 33 + 1
        path = eng.get_path(s, d)
        one = eng.path_load([s], [d], np.array([big], U64))
        assert int(one["totals"][2]) == big * (len(path) - 1)
        for k in range(1, len(path)):
            assert int(one["arc"][eng.find_arc(path[k - 1], path[k])]) == big
        assert int(one["vertex"][d]) == big
    shim.close()
    eng.close()
