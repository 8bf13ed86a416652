"""The small graphs of the batch order 2 tests (tests/test_plan_cost.py on the
host, tests/test_gpu_batch_plan.py on the batched kernels)."""
import numpy as np

from shdpe import generators as G
from shdpe.graph import Topology


def with_isolated_vertex(top):
    """`top` plus one vertex that has a self-loop and no other edge."""
    v = top.n
    return Topology(n=v + 1, directed=top.directed, src=np.append(top.src, v), dst=np.append(top.dst, v),
                    latency=np.append(top.latency, 1.0), loss=np.append(top.loss, 0.0),
                    name=top.name + "_isolated")


def plan_cost_graphs():
    """(name, topology, attached): 3 hubs in 3 of the 16 groups; one hub;
    directed; an attached vertex that no hub reaches.  Latencies are
    continuous (tie-free), no attached count is a multiple of 8."""
    iso = with_isolated_vertex(G.random_sparse(500, 5, seed=12))
    return [
        ("ba1200", G.power_law(1200, m=3, seed=4), G.sample_attached(1200, 300, seed=2)),
        ("ba300", G.power_law(300, m=2, seed=6), G.sample_attached(300, 101, seed=4)),
        ("directed", G.random_sparse(400, 4, seed=7, directed=True), G.sample_attached(400, 150, seed=1)),
        ("isolated", iso, np.append(G.sample_attached(500, 122, seed=8), 500).astype(np.int32)),
    ]
