"""The graphs and the row comparison shared by tests/test_gpu_post_split.py
(the batched post kernel as one kernel and as two) and tests/test_gpu_rounds.py
(the same launches over several rounds).

Graphs: the recipe of tests/test_gpu_pred_filter.py (ba1200 has a degree-114
vertex: the heavy list of the predecessor part; `directed` its own in-lists;
`ties` many tie rows: the deferred tie export and the exact kernel)."""
import numpy as np

from plan_cost_cases import plan_cost_graphs
from shdpe import generators as G
from shdpe.graph import Topology

FIELDS = ("lat", "rel", "hops", "flags", "pred")
FLAG_SEM = 0x07


def _cases():
    # (third: True = no row leaves the batched path; False = tie rows must
    # occur; None = quantised, ties as they fall)
    c = {name: (top, np.asarray(att, np.int32), True) for name, top, att in plan_cost_graphs()}
    mid = G.random_sparse(300, 36, seed=21)
    c["middeg"] = (mid, G.sample_attached(300, 77, seed=3).astype(np.int32), True)
    c["ba1200q"] = (G.power_law(1200, m=3, seed=4, quantum=0.005),
                    G.sample_attached(1200, 300, seed=2).astype(np.int32), None)
    c["ties"] = (G.random_sparse(500, 5, seed=36, quantum=1.0), np.arange(0, 500, 2, dtype=np.int32), False)
    multi = G.with_parallel_edges(G.random_sparse(400, 5, seed=41, vloss=True), 0.3, seed=7)
    c["multigraph"] = (multi, np.arange(0, 400, 3, dtype=np.int32), True)
    return c


CASES = _cases()


def chain(n, seed):
    """Path graph 0-1-...-(n-1) with self-loops: one tree, depth up to n-1
    (a copy of tests/test_gpu_parity.py's)."""
    rng = np.random.default_rng(seed)
    src = np.concatenate([np.arange(n - 1), np.arange(n)])
    dst = np.concatenate([np.arange(1, n), np.arange(n)])
    m = src.shape[0]
    return Topology(n, False, src, dst, rng.uniform(1.0, 50.0, m), rng.uniform(0.0, 0.02, m), None)


def ladder(k, seed):
    """Two chains 0..k-1 and k..2k-1 with rungs i <-> k+i, all latencies 1:
    every row is a tie row, with trees of depth up to ~k (a copy of
    tests/test_gpu_parity.py's, without vertex loss)."""
    rng = np.random.default_rng(seed)
    a = np.arange(k - 1)
    src = np.concatenate([a, a + k, np.arange(k), np.arange(2 * k)])
    dst = np.concatenate([a + 1, a + 1 + k, np.arange(k) + k, np.arange(2 * k)])
    m = src.shape[0]
    return Topology(2 * k, False, src, dst, np.ones(m), rng.uniform(0.0, 0.02, m), None)


def check_rows(rows, exp, ctx):
    ok = (exp["flags"] & 0x03) == 0                # (failed entries carry no values)
    # the flags the oracle knows: unreachable | no edge | zero latency (F_EXACT marks the rows the
    # exact kernel wrote: engine-side, as in tests/test_gpu_sizes.py)
    assert np.array_equal(rows["flags"] & FLAG_SEM, exp["flags"] & FLAG_SEM), ctx
    for k in ("lat", "rel"):
        assert np.array_equal(rows[k][ok].view(np.int64), exp[k][ok].view(np.int64)), (ctx, k)
    for k in ("hops", "pred"):
        assert np.array_equal(rows[k][ok], exp[k][ok]), (ctx, k)
