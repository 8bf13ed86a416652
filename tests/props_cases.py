"""Cases and reference answers of the graph property check
(shd_pe_graph_props / shd_pe_graph_props_host), shared by tests/test_props.py
(CPU) and tests/test_gpu_props.py.

The reference for clusters is scipy.sparse.csgraph.connected_components
(strong for directed graphs, weak for undirected ones), labels canonicalised
to the smallest vertex id of each cluster; the reference for completeness is
a numpy restatement of _topology_isComplete (topology.c:450-552).
"""
import functools

import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

from shdpe.graph import Topology


def _top(n, directed, src, dst, name):
    src = np.asarray(src, dtype=np.int32).reshape(-1)
    dst = np.asarray(dst, dtype=np.int32).reshape(-1)
    m = src.shape[0]
    # latencies / losses only matter where an engine is created from the case
    return Topology(n=n, directed=directed, src=src, dst=dst, latency=1.0 + 0.001 * np.arange(m),
                    loss=np.zeros(m), name=name)


def _pairs(n, directed, self_loops=True):
    """Every ordered (directed) or unordered pair, grouped by source as a
    GraphML writer lists them, then the self-loops."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    keep = (i != j) if directed else (i < j)
    src, dst = i[keep], j[keep]
    if self_loops:
        src = np.concatenate([src, np.arange(n)])
        dst = np.concatenate([dst, np.arange(n)])
    return src, dst


def _ring(ids):
    ids = np.asarray(ids)
    return ids, np.roll(ids, -1)


def _random_multigraph(n, m, rng):
    return rng.integers(0, n, m), rng.integers(0, n, m)


# edge counts of the size cases: neither a multiple of 64 (the last wave of the
# edge loop is partial) nor of 256 (so is the last workgroup)
SIZE_EDGES = {1: 3, 2: 5, 63: 100, 64: 130, 65: 131, 257: 600, 5000: 12345}


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Topology, in a fixed order."""
    out = {}

    def add(name, n, directed, src, dst):
        assert name not in out
        out[name] = _top(n, directed, src, dst, name)

    # sizes: random multigraphs (self-loops and duplicates as they fall)
    for n, m in SIZE_EDGES.items():
        assert m % 64 and m % 256
        for directed in (False, True):
            rng = np.random.default_rng(1000 + n + int(directed))
            add(f"size{n}_{'d' if directed else 'u'}", n, directed, *_random_multigraph(n, m, rng))

    # single vertex
    add("one_noedge_u", 1, False, [], [])
    add("one_noedge_d", 1, True, [], [])
    add("one_loop_u", 1, False, [0], [0])
    add("one_loop_d", 1, True, [0], [0])

    # ---- undirected ----
    rng = np.random.default_rng(11)
    p = rng.permutation(40)                                 # 0..39: a permuted path plus chords
    a = np.concatenate([p[:-1], rng.integers(0, 40, 30)])
    b = np.concatenate([p[1:], rng.integers(0, 40, 30)])
    c = 40 + np.arange(59)                                  # 40..99: a path, the larger component
    add("u_two_components", 100, False, np.concatenate([a, c]), np.concatenate([b, c + 1]))
    s, d = _ring(np.arange(70))
    add("u_isolated_last", 71, False, s, d)                 # vertex 70 has no edge
    perm = np.random.default_rng(12).permutation(300)       # neighbours on the path are far apart in id
    add("u_path_permuted", 300, False, perm[:-1], perm[1:])
    # n = 6: vertex 0 has three self-loops and one other edge: 2*3 + 1 - 1 = 6 >= 6 only if the
    # correction is -1 once (-1 per loop gives 4); the others reach 6 with parallel edges
    s5, d5 = _pairs(5, False)
    add("u_selfloops_parallel", 6, False,
        np.concatenate([[0, 0, 0, 0], s5 + 1, [2, 4]]), np.concatenate([[0, 0, 0, 1], d5 + 1, [3, 5]]))

    # ---- directed ----
    s, d = _ring(np.arange(257))
    add("d_ring257", 257, True, s, d)
    s2, d2 = s.copy(), d.copy()
    s2[100], d2[100] = d[100], s[100]
    add("d_ring257_one_reversed", 257, True, s2, d2)
    add("d_chain500", 500, True, np.arange(499), np.arange(1, 500))
    ra, rb = _ring(np.arange(130)), _ring(130 + np.arange(130))
    add("d_two_rings", 260, True, np.concatenate([ra[0], rb[0], [17]]), np.concatenate([ra[1], rb[1], [200]]))
    k = np.arange(200)
    add("d_two_cycles_chained", 400, True,
        np.concatenate([2 * k, 2 * k + 1, 2 * k[1:]]),       # pair k: 2k <-> 2k+1; pair k+1 -> pair k
        np.concatenate([2 * k + 1, 2 * k, 2 * k[:-1] + 1]))
    rng = np.random.default_rng(7)
    loops = dups = 0
    for tag, m in (("1p5n", 3000), ("2n", 4000), ("4n", 8000)):
        s, d = _random_multigraph(2000, m, rng)
        loops += int((s == d).sum())
        dups += m - len(set(zip(s.tolist(), d.tolist())))
        add(f"d_random2000_{tag}", 2000, True, s, d)
    assert loops and dups                                   # self-loops and duplicates are present
    # five planted strongly connected blocks (a ring plus chords each), joined one way 4 -> 3 -> ... -> 0
    rng = np.random.default_rng(13)
    sizes, src, dst, base = (50, 7, 120, 33, 90), [], [], 0
    firsts = []
    for sz in sizes:
        ids = base + rng.permutation(sz)
        s, d = _ring(ids)
        src += [s, base + rng.integers(0, sz, sz)]
        dst += [d, base + rng.integers(0, sz, sz)]
        firsts.append(base)
        base += sz
    for blk in range(1, 5):
        src.append(np.array([firsts[blk], firsts[blk] + 1]))
        dst.append(np.array([firsts[blk - 1], firsts[blk - 1] + 2]))
    add("d_planted_blocks", base, True, np.concatenate(src), np.concatenate(dst))

    # ---- complete graphs ----
    for n in (64, 65):
        for directed in (False, True):
            t = "d" if directed else "u"
            s, d = _pairs(n, directed)
            add(f"complete{n}_{t}", n, directed, s, d)
            add(f"complete{n}_{t}_minus_edge", n, directed, np.delete(s, 37), np.delete(d, 37))
            add(f"complete{n}_{t}_no_loops", n, directed, *_pairs(n, directed, self_loops=False))
    return out


def canonical_membership(top):
    """scipy's components with every label replaced by its cluster's smallest
    vertex id."""
    n = top.n
    A = sp.coo_matrix((np.ones(top.m, np.int8), (top.src, top.dst)), shape=(n, n)).tocsr()
    if top.directed:
        _, lab = connected_components(A, directed=True, connection="strong")
    else:
        _, lab = connected_components(A, directed=False)
    mn = np.full(lab.max() + 1, n, np.int64)
    np.minimum.at(mn, lab, np.arange(n))
    return mn[lab].astype(np.int32)


def complete_restated(top):
    """_topology_isComplete (topology.c:450-552): per vertex the size of
    igraph_incident(v, IGRAPH_OUT) (:495; an undirected graph lists a self-loop
    twice), minus one when the graph is undirected and edge (v, v) exists
    (:508-520); the first vertex with fewer than vcount ends the walk (:523-530).
    -> (isComplete, firstIncomplete or -1)."""
    n = top.n
    src, dst = top.src.astype(np.int64), top.dst.astype(np.int64)
    ecount = np.bincount(src, minlength=n)
    if not top.directed:
        ecount = ecount + np.bincount(dst, minlength=n)
        has_loop = np.zeros(n, np.int64)
        has_loop[src[src == dst]] = 1
        ecount = ecount - has_loop
    short = np.flatnonzero(ecount < n)
    return (0, int(short[0])) if short.size else (1, -1)


@functools.lru_cache(maxsize=None)
def expected(name):
    """The reference answer of a case: the ShdPeGraphProps fields and the
    membership (computed once, read-only)."""
    top = cases()[name]
    mem = canonical_membership(top)
    mem.setflags(write=False)
    complete, first = complete_restated(top)
    sizes = np.bincount(mem, minlength=top.n)
    clusters = int((sizes > 0).sum())
    return {"isDirected": int(top.directed), "isConnected": int(clusters == 1), "clusterCount": clusters,
            "largestCluster": int(sizes.max()), "isComplete": complete, "firstIncomplete": first,
            "membership": mem}


FIELDS = ("isDirected", "isConnected", "clusterCount", "largestCluster", "isComplete", "firstIncomplete")


def assert_props(got, want, what):
    for f in FIELDS:
        assert got[f] == want[f], (what, f, got[f], want[f])
    if "membership" in got:
        assert np.array_equal(got["membership"], want["membership"]), (what, "membership")
