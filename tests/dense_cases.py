"""Case builders for the dense min-plus path's edge tests (plain helper
module, no tests in here): test_dense_cases.py checks each case's premise
against the oracle on the CPU, test_gpu_dense.py runs them through mode 3.

build(name)            -> (Topology, attached, force_mode); deterministic.
directed_dense(...)    the directed, not complete dense generator.
tie_rows(og, top, srcs) sources whose row k_minplus<PRED> would flag: some
                       v != s has two tight in-arcs u (d[u] + w(u, v) == d[v])
                       of equal minimal d[u].  From the oracle's distances.
"""
import numpy as np

from shdpe import generators as G
from shdpe.graph import Topology

TINY_N = (1, 2, 15, 16, 17)          # K chunk (16) partial / full / one over, one row and column tile
EDGE_N = (127, 128, 129, 257)        # column tile (128) and K chunk remainders 15 / 0 / 1
ROWS_K = (31, 32, 33, 95, 96, 97)    # PRED (32) and SWEEP (96) row tile heights
CHAIN_N = 400


def directed_dense(n, seed, quantum=0.0, loops_missing=0, isolate=0, p=0.6):
    """Directed dense graph: each ordered pair (u, v), u != v, is an arc with
    probability p; latencies lognormal(ln 60, 0.8) clipped to [1, 2000] as in
    G.dense, rounded to multiples of `quantum` (at least one) if given; edge
    and vertex loss U[0, 0.05]; self-loops on every vertex but the first
    `loops_missing`; the last `isolate` vertices have no in-arc from the
    others (unreachable from them)."""
    rng = np.random.default_rng(seed)
    keep = rng.random((n, n)) < p
    np.fill_diagonal(keep, False)
    if isolate:
        keep[:n - isolate, n - isolate:] = False
    src, dst = np.nonzero(keep)
    loops = np.arange(loops_missing, n)
    src, dst = np.concatenate([src, loops]), np.concatenate([dst, loops])
    lat = np.clip(rng.lognormal(np.log(60.0), 0.8, size=src.shape[0]), 1.0, 2000.0)
    if quantum > 0:
        lat = np.maximum(np.round(lat / quantum), 1.0) * quantum
    return Topology(n=n, directed=True, src=src, dst=dst, latency=lat,
                    loss=rng.uniform(0.0, 0.05, size=src.shape[0]),
                    vloss=rng.uniform(0.0, 0.05, size=n),
                    name=f"dirdense{n}_s{seed}" + (f"_q{quantum}" if quantum else ""))


def dense300q():
    """The graph of test_dense_early_stop_tie_rows (one dense chunk by default)."""
    return G.dense(300, seed=3, drop_edge=True, quantum=1.0)


def _chain400():
    from test_gpu_parity import _chain
    return _chain(CHAIN_N, seed=CHAIN_N, vloss=True)


def holes_attached(n=257, isolate=3, loops_missing=5):
    return np.unique(np.concatenate([np.arange(0, n, 3), np.arange(n - isolate, n),
                                     np.arange(loops_missing)])).astype(np.int32)


# name -> (graph, attached (None: every vertex), force_mode)
_CASES = {
    # (n <= 2 without self-loops: with them igraph counts every vertex of such
    # a graph as adjacent to all n, and the graph is complete)
    **{f"tiny_{n}": (lambda n=n: G.random_sparse(n, 4, seed=n, self_loops=n > 2), None, 4)
       for n in TINY_N},
    **{f"edge_{n}": (lambda n=n: G.dense(n, seed=n, drop_edge=True), None, 0) for n in EDGE_N},
    "dir129": (lambda: directed_dense(129, seed=1), None, 0),
    "dir129q": (lambda: directed_dense(129, seed=2, quantum=25.0), None, 0),
    "dir257q_holes": (lambda: directed_dense(257, seed=3, quantum=25.0, loops_missing=5, isolate=3),
                      holes_attached(), 0),
    "und97q": (lambda: G.dense(97, seed=4, drop_edge=True, quantum=25.0), np.arange(0, 97, 2), 0),
    "sparse_q": (lambda: G.random_sparse(300, 6, seed=45, quantum=1.0), None, 4),
    "sparse_dir_q": (lambda: G.random_sparse(300, 6, seed=46, quantum=1.0, directed=True), None, 4),
    "dense300q": (dense300q, None, 0),
    "chain400": (_chain400, None, 4),
}

TINY = [f"tiny_{n}" for n in TINY_N]
EDGE = [f"edge_{n}" for n in EDGE_N]
TIE_UNDIRECTED = ["und97q", "sparse_q", "dense300q"]      # early-stop form (one dense chunk)
TIE_DIRECTED = ["dir129q", "dir257q_holes", "sparse_dir_q"]   # general form, no tie slots
TIE_FREE = ["dir129"]
SIZES = TINY + EDGE + ["dir129", "dir129q", "dir257q_holes", "und97q", "sparse_q", "sparse_dir_q"]
ALL = list(_CASES)


def build(name):
    make, att, force = _CASES[name]
    top = make()
    att = np.arange(top.n, dtype=np.int32) if att is None else np.asarray(att, np.int32)
    return top, att, force


def arc_matrix(top):
    """W[u][v] = latency of arc u -> v (+inf: none; +inf on the diagonal, a
    self-loop never relaxes).  Simple graphs only."""
    W = np.full((top.n, top.n), np.inf)
    W[top.src, top.dst] = top.latency
    if not top.directed:
        W[top.dst, top.src] = top.latency
    np.fill_diagonal(W, np.inf)
    return W


def distances(og, src):
    """The oracle's distance row of `src` over every vertex (+inf: unreached)."""
    d, _, _ = og.raw(int(src), np.arange(og.n, dtype=np.int32))
    return np.where(d < 0, np.inf, d)


def is_tie_row(W, d, s):
    cand = d[:, None] + W                                  # cand[u][v]
    tight = (cand == d[None, :]) & np.isfinite(d)[None, :]
    du = np.where(tight, d[:, None], np.inf)
    best = du.min(axis=0)
    twice = (tight & (du == best[None, :])).sum(axis=0) >= 2
    twice[s] = False
    return bool(twice.any())


def tie_rows(og, top, sources):
    W = arc_matrix(top)
    return [int(s) for s in sources if is_tie_row(W, distances(og, s), int(s))]
