"""The two delta-stepping kernels across their variants: k_sparse_rows in its
four LDS layouts, lanes-per-vertex instantiations, kflags, workgroup sizes and
heavy thresholds, k_batch_rows at 8 and 16 lanes, each over bucket widths from
D0/64 to a single bucket and over latency spreads from uniform to seven
decades -- rows against the CPU oracle, bit for bit.

Every case asserts from shd_pe_sparse_info and the stats that the engine runs
the variant the case names (a mistyped switch would leave the default), and
that the rows came out of the fast kernels and not out of the safety nets
(a tie-free case has no exact rows; a quantised one only early-stop tie rows):
a batch that fails its Bellman check is recomputed by the exact emulation and
would pass parity alone.

Widths are relative to D0, the width a default engine picks for the graph.
No case passes a width below maxdist * 2**-40: widths at which the bucket
bound of the kernels before pe_bucket.hpp stalled are tested on the CPU only
(tests/test_bucket_bound.py).
"""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest

from shdpe import generators as G
from shdpe.graph import Topology
from test_gpu_parity import _assert_rows_equal

pytestmark = pytest.mark.gpu

WIDTHS = ("d64", "d8", "d1", "x8", "single")       # D0/64, D0/8, D0 (explicit), 8*D0, one bucket
FIELDS = ("lat", "rel", "hops", "pred", "flags")
KNOBS = ("SHDPE_LAYOUT", "SHDPE_BATCH", "SHDPE_HEAVY_DEG", "SHDPE_THREADS", "SHDPE_KFLAGS", "SHDPE_DELTA_FACTOR",
         "SHDPE_BATCH_DELTA_FACTOR", "SHDPE_BATCH_LB")
SPARSE, BATCHED = 1, 5                                # forceMode


@pytest.fixture(scope="module")
def E():
    from shdpe import engine
    engine.load_library()
    return engine


@functools.lru_cache(maxsize=None)
def graph(name):
    """(topology, attached, sources, tie-free?)"""
    if name == "A":
        top = G.random_sparse(1500, 5, seed=701)
    elif name == "B":       # A's topology, latencies log-uniform over seven decades
        a = graph("A")[0]
        lat = 10.0 ** np.random.default_rng(702).uniform(-3.0, 4.0, size=a.m)
        top = Topology(n=a.n, directed=False, src=a.src, dst=a.dst, latency=lat, loss=a.loss, vloss=a.vloss,
                       name="rand1500_loguniform")
    elif name == "C":
        top = G.random_sparse(1200, 5, seed=703, directed=True, vloss=True)
    elif name == "D":
        top = G.power_law(3000, m=3, seed=704)
    elif name == "E":
        top = G.random_sparse(800, 6, seed=705, quantum=1.0)
    elif name == "Q2":      # layout 2's light queue (2,396 entries) against BFS levels of thousands
        top = G.random_sparse(10_000, 6, seed=706)
    elif name == "Q2a":     # ... at a size where configure_sparse picks layout 2 by itself (2,132 entries)
        top = G.random_sparse(10_150, 6, seed=708)
    elif name == "Q1":      # layout 1's
        top = G.random_sparse(17_000, 6, seed=707)
    else:
        raise KeyError(name)
    if name.startswith("Q"):
        att = G.sample_attached(top.n, 256, seed=11)
        srcs = att[::32]                              # 8 sources
    else:
        att = np.arange(top.n, dtype=np.int32)
        srcs = G.sample_attached(top.n, 32, seed=12)
    return top, att, srcs, name != "E"


@functools.lru_cache(maxsize=None)
def oracle_rows(name):
    """The oracle's rows of the graph's sources, and its largest finite distance."""
    import oracle
    oracle.build()
    top, att, srcs, _ = graph(name)
    og = oracle.OracleGraph(top)
    exp = og.rows(srcs, att, threads=8)
    maxdist = 0.0
    every = np.arange(top.n, dtype=np.int32)
    for s in srcs:
        d = og.raw(int(s), every)[0]
        maxdist = max(maxdist, float(d[np.isfinite(d)].max()))
    for v in exp.values():
        v.setflags(write=False)
    return exp, maxdist


def _degrees(top):
    """Out-arcs per vertex without self-loops (what the heavy threshold is compared with)."""
    keep = top.src != top.dst
    deg = np.bincount(top.src[keep], minlength=top.n)
    if not top.directed:
        deg = deg + np.bincount(top.dst[keep], minlength=top.n)
    return deg


@functools.lru_cache(maxsize=None)
def bfs_levels(name):
    """Hop distance of every vertex from the graph's first source."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import shortest_path
    top, _, srcs, _ = graph(name)
    g = sp.coo_matrix((np.ones(top.m), (top.src, top.dst)), shape=(top.n, top.n)).tocsr()
    h = shortest_path(g, directed=top.directed, unweighted=True, indices=int(srcs[0]))
    assert np.isfinite(h).all()
    return h.astype(np.int64)


def largest_level(name, heavy_deg, heavy):
    """The largest BFS level of the first source, counting heavy (degree >=
    heavy_deg) or light vertices only.  With one bucket the relax loops are
    Bellman-Ford sweeps: while no queue has overflowed, sweep k's frontier holds
    level k whole, so a level above the capacity takes the overflow branch."""
    deg = _degrees(graph(name)[0])
    sel = deg >= heavy_deg if heavy else deg < heavy_deg
    return int(np.bincount(bfs_levels(name)[sel]).max())


class _env:
    def __init__(self, env):
        self.env = {k: str(v) for k, v in env}
        assert set(self.env) <= set(KNOBS), self.env

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in KNOBS}
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


_D0 = {}


def d0(E, name, kernel):
    """deltaUsed of a default engine of this kernel on the graph."""
    if (name, kernel) not in _D0:
        top, att, _, _ = graph(name)
        with _env(()):
            eng = E.Engine(top, att, force_mode=kernel)
            _D0[name, kernel] = eng.stats()["deltaUsed"]
            eng.close()
    assert _D0[name, kernel] > 0
    return _D0[name, kernel]


def width_value(E, name, kernel, width):
    """The option's value for a named width (0.0 = automatic)."""
    if width == "auto":
        return 0.0
    maxdist = oracle_rows(name)[1]
    if width == "single":
        delta = 2.0 * maxdist
    else:
        delta = d0(E, name, kernel) * {"d64": 1 / 64, "d8": 1 / 8, "d1": 1.0, "x8": 8.0}[width]
    # never a width at which the bucket bound could fail to advance
    assert delta >= maxdist * 2.0 ** -40, (name, width, delta, maxdist)
    return delta


_RUNS = {}


def run(E, name, kernel, width="auto", env=()):
    """One engine over the graph's sources: its raw rows, stats and sparse
    launch.  Memoised: the width-independence tests read the parity cases'."""
    key = (name, kernel, width, tuple(env))
    if key in _RUNS:
        return _RUNS[key]
    top, att, srcs, _ = graph(name)
    delta = width_value(E, name, kernel, width)
    with _env(env):
        eng = E.Engine(top, att, delta=delta, force_mode=kernel, debug_flags=E.DEBUG_ENV)
        info = eng.sparse_info()
        eng.compute_rows(srcs)
        got = [eng.get_row(int(s)) for s in srcs]
        st = eng.stats()
        eng.close()
    rows = {k: np.stack([g[k] for g in got]) for k in FIELDS}
    for v in rows.values():
        v.setflags(write=False)
    r = SimpleNamespace(rows=rows, st=st, info=info, delta=delta, key=key)
    _RUNS[key] = r
    print(f"{key}: delta {st['deltaUsed']:.6g} sparse_info {info} batched {st['batched']} lanes {st['batchLanes']} "
          f"exact {st['rowsExact']} tieEarly {st['rowsTieEarly']} repaired {st['rowsTieRepaired']}")
    return r


def check(E, name, kernel, width="auto", env=(), fast=True, **want):
    """Run, then: the engine ran what the case names (`want`: sparse_info
    entries, or batchLanes), the rows are the oracle's, and -- unless fast is
    False -- they came from the fast path."""
    r = run(E, name, kernel, width, env)
    ctx = str(r.key)
    exp, _ = oracle_rows(name)
    srcs, tiefree = graph(name)[2:]
    # the variant
    assert r.st["mode"] == 1 and r.st["batched"] == (1 if kernel == BATCHED else 0), ctx
    if width == "auto":
        assert r.st["deltaUsed"] == d0(E, name, kernel) or any(k.endswith("DELTA_FACTOR") for k, _ in env), ctx
    else:
        assert r.st["deltaUsed"] == r.delta, ctx
    for k, v in want.items():
        have = r.st["batchLanes"] if k == "batchLanes" else r.info[k]
        assert have == v, f"{ctx}: {k} is {have}, the case wants {v}"
    # parity
    for i, s in enumerate(srcs):
        _assert_rows_equal({k: r.rows[k][i] for k in FIELDS}, {k: v[i] for k, v in exp.items()}, f"{ctx} row {s}")
    # the fast path
    assert r.st["rowsComputed"] == len(srcs), ctx
    assert r.st["rowsTieRepaired"] == 0, f"{ctx}: {r.st}"
    if fast:
        if tiefree:
            assert r.st["rowsExact"] == 0, f"{ctx}: rows left the fast path: {r.st}"
        else:
            assert r.st["rowsExact"] == r.st["rowsTieEarly"] > 0, f"{ctx}: full-emulation rows: {r.st}"
    return r


def layout_env(layout):
    return (("SHDPE_LAYOUT", layout),) + ((("SHDPE_BATCH", 0),) if layout == 0 else ())


# ---- k_sparse_rows ---------------------------------------------------------

@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("layout", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["A", "B"])
def test_sparse_layouts_and_widths(E, name, layout, width):
    check(E, name, SPARSE, width, layout_env(layout), layout=layout, lanesPerVertex=4, heavyDeg=64, threads=512,
          kflags=0)


@pytest.mark.parametrize("layout", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["C", "E"])
def test_sparse_layouts_directed_and_ties(E, name, layout):
    """C: the in-arc scan of process_group and the general reliability fold;
    E: the tie export, which every layout writes from its own arrays."""
    check(E, name, SPARSE, "auto", layout_env(layout), layout=layout)


@pytest.mark.parametrize("width", ["auto", "single"])
@pytest.mark.parametrize("layout", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["A", "D"])
def test_sparse_heavy_queue_overflow(E, name, layout, width):
    """Threshold 2: every vertex but a path's ends goes through the heavy
    queue (one wave per vertex), whose 256 entries a BFS level exceeds."""
    r = check(E, name, SPARSE, width, layout_env(layout) + (("SHDPE_HEAVY_DEG", 2),), layout=layout, heavyDeg=2)
    level = largest_level(name, 2, heavy=True)
    print(f"{r.key}: largest heavy BFS level {level} against hcap {r.info['hcap']}")
    assert level > r.info["hcap"]


@pytest.mark.parametrize("threads", [64, 256])
@pytest.mark.parametrize("layout", [0, 2])
def test_sparse_threads(E, layout, threads):
    check(E, "A", SPARSE, "auto", layout_env(layout) + (("SHDPE_THREADS", threads),), layout=layout, threads=threads)


@pytest.mark.parametrize("kflags,lpv", [(16, 2), (32, 1), (48, 8)])
def test_sparse_lanes_per_vertex(E, kflags, lpv):
    check(E, "A", SPARSE, "auto", layout_env(3) + (("SHDPE_KFLAGS", kflags),), layout=3, kflags=kflags,
          lanesPerVertex=lpv)


@pytest.mark.parametrize("kflags", [1, 2, 4, 8])
def test_sparse_kflags(E, kflags):
    """The SoA arc loads of the relax (1), the row writer's streaming stores (4),
    the grouped predecessor pass (8) and bit 2, which pe_device.hpp names and
    no kernel reads today, at the automatic layout."""
    auto = run(E, "A", SPARSE).info["layout"]
    check(E, "A", SPARSE, "auto", (("SHDPE_KFLAGS", kflags),), layout=auto, kflags=kflags, lanesPerVertex=4)


def test_sparse_width_by_factor(E):
    """SHDPE_DELTA_FACTOR in place of the option: 16 -> 2 is D0/8 exactly."""
    r = check(E, "A", SPARSE, "auto", (("SHDPE_DELTA_FACTOR", 2),))
    assert r.st["deltaUsed"] == d0(E, "A", SPARSE) / 8
    same = run(E, "A", SPARSE, "d8")
    for k in FIELDS:
        assert r.rows[k].tobytes() == same.rows[k].tobytes(), k


@pytest.mark.parametrize("name,layout,auto", [("Q2", 2, 3), ("Q2a", 2, 2), ("Q1", 1, 1)])
def test_sparse_light_queue_overflow(E, name, layout, auto):
    """The LDS light queues at the smallest sizes where a frontier exceeds
    them, one bucket: layout 2 at n = 10,000 (where two rows per CU make
    layout 3 the automatic one, so it is asked for) and at n = 10,150, layout
    1 at n = 17,000 (both automatic)."""
    assert run(E, name, SPARSE).info["layout"] == auto
    env = () if auto == layout else layout_env(layout)
    r = check(E, name, SPARSE, "single", env, layout=layout, heavyDeg=64)
    level = largest_level(name, 64, heavy=False)
    print(f"{r.key}: automatic layout {auto}; largest light BFS level {level} against qcap {r.info['qcap']}")
    assert level > r.info["qcap"]


# ---- k_batch_rows ----------------------------------------------------------

def batch_fast(E, name, width):
    """Whether the arithmetic keeps a batch below its phase cap (8n + 1024):
    4 x the largest distance / delta < 8n.  Small widths that miss it may take
    the cap's way out (correct, slower): parity only."""
    if width == "auto":
        return True
    top = graph(name)[0]
    return 4.0 * oracle_rows(name)[1] / width_value(E, name, BATCHED, width) < 8 * top.n


@pytest.mark.parametrize("heavy", [None, 2])
@pytest.mark.parametrize("width", ["d8", "d1", "x8", "single"])
@pytest.mark.parametrize("lb", [8, 16])
def test_batched_lanes_widths_threshold(E, lb, width, heavy):
    env = (("SHDPE_BATCH_LB", lb),) + ((("SHDPE_HEAVY_DEG", heavy),) if heavy else ())
    assert batch_fast(E, "A", width)          # the precondition of the fast-path assertion
    check(E, "A", BATCHED, width, env, batchLanes=lb, heavyDeg=heavy or 64)


@pytest.mark.parametrize("width", ["auto", "single"])
@pytest.mark.parametrize("name", ["B", "D", "E"])
def test_batched_other_graphs(E, name, width):
    assert batch_fast(E, name, width)
    check(E, name, BATCHED, width)


def test_batched_width_by_factor(E):
    """SHDPE_BATCH_DELTA_FACTOR in place of the option: 0.75 -> 0.09375 is D0/8 exactly."""
    assert batch_fast(E, "A", "d8")
    r = check(E, "A", BATCHED, "auto", (("SHDPE_BATCH_DELTA_FACTOR", 0.09375),))
    assert r.st["deltaUsed"] == d0(E, "A", BATCHED) / 8
    same = check(E, "A", BATCHED, "d8")
    for k in FIELDS:
        assert r.rows[k].tobytes() == same.rows[k].tobytes(), k


# ---- width independence, GPU against GPU -----------------------------------

@pytest.mark.parametrize("kernel", [SPARSE, BATCHED], ids=["sparse", "batched"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_rows_do_not_depend_on_the_width(E, name, kernel):
    """Every width's raw rows are the automatic width's, byte for byte (on top
    of the oracle comparison: a failure here says which side moved)."""
    envs = [layout_env(layout) for layout in (0, 1, 2, 3)] if kernel == SPARSE else [()]
    for env in envs:
        base = run(E, name, kernel, "auto", env)
        for width in WIDTHS:
            r = check(E, name, kernel, width, env, fast=kernel == SPARSE or batch_fast(E, name, width))
            for k in FIELDS:
                assert r.rows[k].tobytes() == base.rows[k].tobytes(), (r.key, k)
