"""The batch plan composed on the device (pe_plan_dev.hip) against the host
planner (batch_order_cost), which SHDPE_DEVICE_PLAN=0 keeps in use.

Every case runs one engine per setting of the switch with SHDPE_DUMP_BATCHES
and compares the two dumps -- the plan the kernels ran with, read back from
the device when the plan kernels made it:

  compositions  the same batches (rows in the same lanes, pads last);
  offsets       bit-equal per batch and lane;
  sequence      the same wherever neighbouring host costs differ by more than
                4 ulp (the device's sqrt is the one operation not known to
                round as the host's; within such a run the same batches in any
                order), and exactly the host's where the costs are equal: the
                order is stable by batch index.

The host costs are restated here in numpy, operation by operation in
batch_order_cost's sequence, from the dump's own distances.  The library says
on stderr who made the plan of each call, so a switch that is silently off
cannot pass.  The table rows of the two runs are byte-identical and bit-exact
against the oracle."""
import contextlib
import os
from types import SimpleNamespace

import numpy as np
import pytest

from device_plan_cases import ba1200, many_batches, two_components, twins
from post_split_cases import FIELDS, check_rows
from shdpe import generators as G

pytestmark = pytest.mark.gpu

SWITCHES = ("SHDPE_DEVICE_PLAN", "SHDPE_BATCH_LB", "SHDPE_BATCH_GRID", "SHDPE_BATCH_ROUND", "SHDPE_DUMP_BATCHES",
            "SHDPE_POST_SPLIT", "SHDPE_LANE_OFFSET")
COST_C0, COST_OFF, COST_SPREAD = 0.892, 0.200, 3.363        # pe_plan.hpp
BY = {0: "host planner", 1: "plan kernels"}


@pytest.fixture(scope="module")
def E():
    from shdpe import engine
    engine.load_library()
    return engine


@pytest.fixture(scope="module")
def ba():
    return ba1200(), G.sample_attached(1200, 300, seed=2)


@pytest.fixture(scope="module")
def ba_expected(oracle_mod, ba):
    """The oracle's table of the 1,200-vertex graph, computed once."""
    top, att = ba
    return oracle_mod.OracleGraph(top).rows(att, att, threads=8)


@contextlib.contextmanager
def switches(env):
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    try:
        for k, v in env.items():
            assert k in SWITCHES, k
            os.environ[k] = str(v)
        yield
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def read_dump(path):
    """SHDPE_DUMP_BATCHES (dump_batches, pe_engine.hip)."""
    with open(path, "rb") as f:
        b = f.read()
    at = [0]

    def take(dtype, count):
        a = np.frombuffer(b, dtype, count, at[0]).copy()
        at[0] += a.nbytes
        return a
    nB, LB = (int(x) for x in take(np.int32, 2))
    d = SimpleNamespace(nB=nB, LB=LB, order=take(np.int32, nB * LB).reshape(nB, LB))
    take(np.int32, nB * 16)                                   # kernel counters
    T = int(take(np.int64, 1)[0])
    d.rowOff = take(np.float64, T)
    G_ = int(take(np.int32, 1)[0])
    mean = float(take(np.float64, 1)[0])
    d.unit = mean if mean > 0.0 and np.isfinite(mean) else 1.0
    d.dist = take(np.float64, T * G_).reshape(T, G_)
    d.laneOff = take(np.float64, nB * LB).reshape(nB, LB)
    assert at[0] == len(b)
    return d


def host_costs(d):
    """batch_order_cost's cost of the dump's batches: every sum in its order
    (per lane ascending, then per group ascending), one rounding per operation."""
    order, nB, LB, nG = d.order, d.nB, d.LB, d.dist.shape[1]
    s, q = np.zeros((nB, nG)), np.zeros((nB, nG))
    c = np.zeros((nB, nG), np.int64)
    off, lanes = np.zeros(nB), np.zeros(nB, np.int64)
    for l in range(LB):
        real = order[:, l] >= 0
        p = np.where(real, order[:, l], 0)
        lanes += real
        off = np.where(real, off + d.rowOff[p], off)
        fin = np.isfinite(d.dist[p]) & real[:, None]
        x = (np.where(fin, d.dist[p], 0.0) - d.rowOff[p][:, None]) / d.unit
        s = np.where(fin, s + x, s)
        q = np.where(fin, q + x * x, q)
        c += fin
    var, terms = np.zeros(nB), np.zeros(nB, np.int64)
    for j in range(nG):
        has = c[:, j] > 0
        t = q[:, j] - s[:, j] * s[:, j] / np.where(has, c[:, j], 1)
        var = np.where(has, var + np.where(t > 0.0, t, 0.0), var)
        terms += c[:, j]
    spread = np.where(terms > 0, np.sqrt(var / np.maximum(terms, 1)), 0.0)
    mean_off = off / lanes / d.unit
    return (COST_C0 + COST_OFF * mean_off + COST_SPREAD * spread) * lanes / LB


def compare_plans(h, d, ctx):
    """The device's dump d against the host's h; returns the host costs."""
    assert (h.nB, h.LB) == (d.nB, d.LB), ctx
    hb = [tuple(r) for r in h.order.tolist()]
    db = [tuple(r) for r in d.order.tolist()]
    assert len(set(hb)) == h.nB
    assert sorted(hb) == sorted(db), (ctx, "compositions")
    for r in hb:                                              # rows first, pads last
        k = sum(x >= 0 for x in r)
        assert k > 0 and all(x >= 0 for x in r[:k]) and all(x == -1 for x in r[k:]), (ctx, r)
    at = {r: i for i, r in enumerate(db)}
    for i, r in enumerate(hb):
        assert h.laneOff[i].tobytes() == d.laneOff[at[r]].tobytes(), (ctx, "offsets", i, h.laneOff[i], d.laneOff[at[r]])
    cost = host_costs(h)
    assert np.all(np.isfinite(cost)) and np.all(cost > 0.0) and np.all(cost[:-1] >= cost[1:]), (ctx, "host costs")
    # runs of host batches whose neighbouring costs are within 4 ulp of each other
    near = np.abs(cost[:-1] - cost[1:]) <= 4.0 * np.spacing(np.maximum(cost[:-1], cost[1:]))
    a = 0
    for i in range(1, h.nB + 1):
        if i < h.nB and near[i - 1]:
            continue
        if np.all(cost[a:i] == cost[a]):                      # equal costs (a run of one too): the host's order
            assert hb[a:i] == db[a:i], (ctx, "sequence", a, i)
        else:
            assert sorted(hb[a:i]) == sorted(db[a:i]), (ctx, "sequence within 4 ulp", a, i)
        a = i
    return cost


def run(E, capfd, tmp_path, top, att, dev, lb=16, env=None, sources=None, shards=None, paths=None):
    """One engine with the switch at `dev`.  The table (or the rows of
    `sources`; with `shards` devices one compute per shard, so each writes a
    dump of its own), the dumps, and who made each call's plan."""
    dump = str(tmp_path / f"dump{dev}.bin")
    env = dict(env or {}, SHDPE_DEVICE_PLAN=dev, SHDPE_BATCH_LB=lb, SHDPE_DUMP_BATCHES=dump)
    r = SimpleNamespace(dumps=[], by=[], paths=None)
    capfd.readouterr()

    def called():
        r.dumps.append(read_dump(dump))
        os.remove(dump)
        err = capfd.readouterr().err
        r.by += [ln.split(" batch plan by the ")[1] for ln in err.splitlines() if " batch plan by the " in ln]

    with switches(env):
        kw = {} if shards is None else {"devices": [0] * shards}
        eng = E.Engine(top, att, force_mode=5, debug_flags=E.DEBUG_ENV | E.DEBUG_COUNTERS, **kw)
        try:
            assert np.array_equal(eng.attached, att)
            r.T = eng.T
            if paths is not None:
                r.paths = eng.get_paths(paths[0], paths[1], hops=True)
                called()
            if sources is not None:
                eng.compute_rows(sources)
                called()
                got = [eng.get_row(int(s)) for s in sources]
                rows = {k: np.stack([g[k] for g in got]) for k in FIELDS}
            else:
                r.bounds = [int(x) for x in eng.shard_bounds()] if shards else [0, eng.T]
                for a, b in zip(r.bounds[:-1], r.bounds[1:]):
                    eng.compute_positions(a, b - a)
                    called()
                rows = eng.get_rows(0, eng.T) if eng.T <= 2048 else None
            r.rows = None if rows is None else {k: rows[k] for k in FIELDS}
            r.sample = {k: np.concatenate([eng.get_rows(p, 1)[k] for p in range(0, eng.T, max(1, eng.T // 64))])
                        for k in FIELDS} if rows is None else None
            r.st = eng.stats()
            r.binfo = [eng.batch_info(i) for i in range(r.st["nShards"])]
        finally:
            eng.close()
    assert r.st["mode"] == 1 and r.st["batched"] == 1 and r.st["batchLanes"] == lb, r.st
    return r


def both(E, capfd, tmp_path, top, att, ctx, **kw):
    """The case with the switch at 0 and at 1: plans compared call by call,
    rows byte for byte.  Returns (host run, device run, host costs per call)."""
    h = run(E, capfd, tmp_path, top, att, 0, **kw)
    d = run(E, capfd, tmp_path, top, att, 1, **kw)
    # shd_pe_get_paths on a fresh engine first computes its sources' rows (a plan of the switch's
    # side), then the path tier runs the batches it composed itself: that call's dump is the tier's
    first = 1 if kw.get("paths") is not None else 0
    for r, dev in ((h, 0), (d, 1)):
        want = [BY[dev], "caller"] * first + [BY[dev]] * (len(r.dumps) - first)
        assert r.by == want, (ctx, dev, r.by)
    assert len(h.dumps) == len(d.dumps)
    for a, b in zip(h.dumps[:first], d.dumps[:first]):
        assert a.order.tobytes() == b.order.tobytes() and a.laneOff.tobytes() == b.laneOff.tobytes(), (ctx, "caller")
    costs = [compare_plans(a, b, f"{ctx} call {i}")
             for i, (a, b) in enumerate(zip(h.dumps[first:], d.dumps[first:]))]
    for k in FIELDS:
        x, y = (h.rows, d.rows) if h.rows is not None else (h.sample, d.sample)
        assert x[k].tobytes() == y[k].tobytes(), (ctx, k)
    assert h.binfo == d.binfo, (ctx, h.binfo, d.binfo)
    assert h.st["rowsExact"] == d.st["rowsExact"] and d.st["rowsTieRepaired"] == 0, (ctx, h.st, d.st)
    return h, d, costs


@pytest.mark.parametrize("lb", [8, 16])
@pytest.mark.parametrize("rows", [300, 40, 16, 1])
def test_table_sizes(E, capfd, tmp_path, oracle_mod, ba, ba_expected, rows, lb):
    """300 rows; 40 rows (no multiple of the lanes); one batch of 16 (two of
    8); one row."""
    top, att = ba
    att = att[:rows]
    h, d, _ = both(E, capfd, tmp_path, top, att, f"ba1200 rows {rows} lb {lb}", lb=lb)
    assert d.dumps[0].nB == -(-rows // lb)
    exp = ba_expected if rows == 300 else oracle_mod.OracleGraph(top).rows(att, att, threads=8)
    check_rows(d.rows, exp, f"rows {rows} lb {lb}")


@pytest.mark.parametrize("lb", [8, 16])
def test_nearest_hub_offsets(E, capfd, tmp_path, ba, ba_expected, lb):
    """SHDPE_LANE_OFFSET=0: every batch's offsets are the nearest-hub
    distances (the plan kernel's kind 0), the sequence the same costs give."""
    top, att = ba
    h, d, _ = both(E, capfd, tmp_path, top, att, f"kind 0 lb {lb}", lb=lb, env={"SHDPE_LANE_OFFSET": 0})
    dump = d.dumps[0]
    real = dump.order >= 0
    want = np.where(real, dump.rowOff[np.where(real, dump.order, 0)], 0.0)
    assert dump.laneOff.tobytes() == want.tobytes()
    check_rows(d.rows, ba_expected, f"kind 0 lb {lb}")


def test_shuffled_subset(E, capfd, tmp_path, ba, ba_expected):
    """101 of the 300 rows in a shuffled order through shd_pe_compute_rows:
    the sort is by (rank, index in the request), whatever the request's order."""
    top, att = ba
    pick = np.random.default_rng(8).permutation(300)[:101]
    h, d, _ = both(E, capfd, tmp_path, top, att, "subset", sources=att[pick])
    assert d.dumps[0].nB == 7 and sorted(d.dumps[0].order[d.dumps[0].order >= 0].tolist()) == sorted(pick.tolist())
    check_rows(d.rows, {k: v[pick] for k, v in ba_expected.items()}, "subset")


@pytest.mark.parametrize("lb", [8, 16])
def test_two_components(E, capfd, tmp_path, oracle_mod, lb):
    """Hub groups that reach no lane of a batch, groups that reach a part of
    one, a batch with no common group (offsets fall back to the nearest-hub
    distance) and a source no hub reaches."""
    top, att = two_components()
    h, d, _ = both(E, capfd, tmp_path, top, att, f"two components lb {lb}", lb=lb)
    dump = d.dumps[0]
    fin = np.isfinite(dump.dist)
    assert (~fin.any(axis=1)).sum() == 1                      # the lone vertex
    real = dump.order >= 0
    reach = np.stack([(fin[np.where(real[b], dump.order[b], 0)] & real[b][:, None]).sum(axis=0) for b in range(dump.nB)])
    lanes = real.sum(axis=1)[:, None]
    assert (reach == 0).any() and ((reach > 0) & (reach < lanes)).any()
    fallback = np.flatnonzero((reach < lanes).all(axis=1))
    assert fallback.shape[0] >= 1
    for b in fallback:                                        # the nearest-hub distances, pads 0
        want = np.where(real[b], dump.rowOff[np.where(real[b], dump.order[b], 0)], 0.0)
        assert dump.laneOff[b].tobytes() == want.tobytes()
    check_rows(d.rows, oracle_mod.OracleGraph(top).rows(att, att, threads=8), f"two components lb {lb}")


@pytest.mark.parametrize("lb", [8, 16])
def test_equal_costs_keep_rank_order(E, capfd, tmp_path, oracle_mod, lb):
    """Identical components: batches with exactly equal costs, in the host's
    (stable) order on the device too."""
    top, att = twins()
    h, d, costs = both(E, capfd, tmp_path, top, att, f"twins lb {lb}", lb=lb)
    assert (costs[0][:-1] == costs[0][1:]).sum() >= 3 * (32 // lb) // 2
    assert h.dumps[0].order.tobytes() == d.dumps[0].order.tobytes()
    check_rows(d.rows, oracle_mod.OracleGraph(top).rows(att, att, threads=8), f"twins lb {lb}")


def test_more_batches_than_one_workgroup_sorts(E, capfd, tmp_path, oracle_mod):
    """1,125 batches of 8: neither sort fits one workgroup's LDS.  (The table
    is 81 M entries: rows are compared on a sample of 65.)"""
    top, att = many_batches()
    h, d, _ = both(E, capfd, tmp_path, top, att, "many batches", lb=8)
    assert d.dumps[0].nB == 1125
    pos = np.arange(0, 9000, 9000 // 64)
    exp = oracle_mod.OracleGraph(top).rows(att[pos], att, threads=8)
    check_rows(d.sample, exp, "many batches")


def test_two_shards(E, capfd, tmp_path, ba, ba_expected):
    """Each shard plans its own rows from its own copy of the inputs."""
    top, att = ba
    h, d, _ = both(E, capfd, tmp_path, top, att, "two shards", lb=8, shards=2)
    assert len(d.dumps) == 2 and d.st["nShards"] == 2 and 0 < d.bounds[1] < 300
    for i, dump in enumerate(d.dumps):
        rows = dump.order[dump.order >= 0]
        assert sorted(rows.tolist()) == list(range(d.bounds[i], d.bounds[i + 1]))
    check_rows(d.rows, ba_expected, "two shards")


def test_several_rounds(E, capfd, tmp_path, ba, ba_expected):
    """One plan, taken in rounds of 3 batches on 2 slots: the control words
    the plan's last kernel sets serve every round."""
    top, att = ba
    for split in (1, 0):
        env = {"SHDPE_BATCH_GRID": 2, "SHDPE_BATCH_ROUND": 3, "SHDPE_POST_SPLIT": split}
        h, d, _ = both(E, capfd, tmp_path, top, att, f"rounds split {split}", lb=8, env=env)
        assert d.binfo[0] == {"perRound": 3, "slots": 2, "rounds": 13, "batches": 38}, d.binfo
        check_rows(d.rows, ba_expected, f"rounds split {split}")


def test_compute_after_attach(E, capfd, tmp_path, oracle_mod, ba):
    """Hosts attached by shd_pe_attach_hosts, an engine over their vertices,
    then another attachment and its engine: each engine's plan comes from the
    ranks and hub distances of its own attached set."""
    top, _ = ba
    va = G.vertex_attrs(top.n, seed=41)
    at = E.Attacher(va)
    seen = []
    try:
        for seed in (1, 2):
            hosts = at.attach(G.attach_hints(va, 150, seed=seed))["vertex"].astype(np.int32)
            att = hosts[np.sort(np.unique(hosts, return_index=True)[1])]     # first occurrences, as the engine keeps them
            h, d, _ = both(E, capfd, tmp_path, top, att, f"attach {seed}")
            check_rows(d.rows, oracle_mod.OracleGraph(top).rows(att, att, threads=8), f"attach {seed}")
            seen.append((att, d.dumps[0]))
    finally:
        at.close()
        va.close()
    assert not np.array_equal(seen[0][0], seen[1][0])
    assert seen[0][1].dist.tobytes() != seen[1][1].dist.tobytes()


def test_get_paths_keeps_the_host_order(E, capfd, tmp_path, ba, ba_expected):
    """shd_pe_get_paths composes its batches itself (batch_order of its unique
    sources) with the switch either way; the compute after it plans on the device."""
    top, att = ba
    rng = np.random.default_rng(5)
    src, dst = rng.choice(att, 60).astype(np.int32), rng.choice(att, 60).astype(np.int32)
    h, d, _ = both(E, capfd, tmp_path, top, att, "paths", lb=8, paths=(src, dst))
    assert d.by == [BY[1], "caller", BY[1]] and len(d.dumps) == 2
    for name, x, y in zip(("offsets", "verts", "status", "hop lat", "hop rel"), d.paths, h.paths):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), name
    assert (np.asarray(d.paths[2]) == 0).sum() > 30
    check_rows(d.rows, ba_expected, "paths")
