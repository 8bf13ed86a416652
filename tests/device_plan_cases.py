"""The small graphs of the device plan tests (tests/test_gpu_device_plan.py on
the plan kernels, tests/test_plan_order_cost.py on the host planner)."""
import numpy as np

from shdpe import generators as G
from shdpe.graph import Topology


def join(*tops):
    """The disjoint union of undirected topologies, vertex ids shifted."""
    off = np.cumsum([0] + [t.n for t in tops])
    return Topology(n=int(off[-1]), directed=False,
                    src=np.concatenate([t.src + o for t, o in zip(tops, off)]).astype(np.int32),
                    dst=np.concatenate([t.dst + o for t, o in zip(tops, off)]).astype(np.int32),
                    latency=np.concatenate([t.latency for t in tops]),
                    loss=np.concatenate([t.loss for t in tops]), name="+".join(t.name for t in tops))


def loop_vertex():
    """One vertex with a self-loop: attached, it is a source that no hub reaches."""
    return Topology(n=1, directed=False, src=np.zeros(1, np.int32), dst=np.zeros(1, np.int32),
                    latency=np.ones(1), loss=np.zeros(1), name="loop")


def ba1200():
    """The Barabasi-Albert graph of the batch plan tests: 3 hubs in 3 of the 16 groups."""
    return G.power_law(1200, m=3, seed=4)


def two_components():
    """1,200 + 900 vertices and a lone vertex: 5 hubs, each reaching one
    component only, so a batch that spans the border between two hubs' cells
    of different components has no common group (its offsets fall back to the
    nearest-hub distances) and the groups reach a part of it."""
    top = join(ba1200(), G.power_law(900, m=3, seed=9), loop_vertex())
    att = np.append(G.sample_attached(2100, 299, seed=3), 2100).astype(np.int32)
    return top, att


TWIN_N, TWIN_COPIES, TWIN_ROWS = 480, 5, 32


def twins():
    """Five copies of one graph of 480 vertices: 6 hubs, the highest-degree
    vertex of every copy and one more in copy 0.  Copies 1 to 4 have the same
    32 attached vertices each and none in copy 0: four cells of 32 rows with
    the same distances to their one hub, so the batches of a cell have exact
    twins in the others and equal costs must keep their rank order."""
    one = G.power_law(TWIN_N, m=3, seed=11)
    top = join(*[one] * TWIN_COPIES)
    local = G.sample_attached(TWIN_N, TWIN_ROWS, seed=5)
    att = np.concatenate([local + TWIN_N * c for c in range(1, TWIN_COPIES)]).astype(np.int32)
    return top, att


def many_batches():
    """More than 1,024 batches at 8 lanes: 9,000 attached vertices of 12,000."""
    return G.power_law(12000, m=3, seed=21), G.sample_attached(12000, 9000, seed=6)
