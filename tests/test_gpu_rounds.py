"""The split batch kernels over several rounds, and a tie batch on a shard
without tie slots.

A round is the batches whose distance arrays persist from the relax to the post
kernel (or its predecessor and label parts and the redo launch), the tie export
and shd_pe_get_paths' walk; every table computed so far fits one round, so the
second iteration of that loop ran nowhere.  SHDPE_BATCH_ROUND=k (tests only)
caps the batches per round, SHDPE_BATCH_GRID=g the scratch slots below it, and
shd_pe_batch_info reports what was run: every test asserts the round count it
claims, so a switch that is silently off cannot pass.  SHDPE_TIE_SLOTS=k caps
the tie slots; 0 is the state of a shard past 2^30 arcs.

Every table is compared bit for bit with the oracle (computed once per module)
and byte for byte with the same engine's one-round run (computed once per
setting).  Graphs and comparison: tests/post_split_cases.py."""
import contextlib
import os
from types import SimpleNamespace

import numpy as np
import pytest

from post_split_cases import CASES, FIELDS, chain, check_rows, ladder
from shdpe.graph import Topology

pytestmark = pytest.mark.gpu

SWITCHES = ("SHDPE_POST_SPLIT", "SHDPE_BATCH_LB", "SHDPE_BATCH_GRID", "SHDPE_BATCH_ROUND", "SHDPE_BATCH_WPE",
            "SHDPE_TIE_SLOTS", "SHDPE_TIE_CORRUPT", "SHDPE_PRED_FILTER", "SHDPE_TUNE_FAIL_WPE")
ROUND_CASES = ("ba1200", "directed", "ties", "multigraph", "ba1200q")
SETTINGS = [(1, 1), (2, 3), (4, 5)]            # (SHDPE_BATCH_GRID, SHDPE_BATCH_ROUND)


@pytest.fixture(scope="module")
def E():
    from shdpe import engine
    engine.load_library()
    return engine


@pytest.fixture(scope="module")
def expected(oracle_mod):
    """The oracle's rows of every case used here, computed once."""
    return {name: oracle_mod.OracleGraph(CASES[name][0]).rows(CASES[name][1], CASES[name][1], threads=8)
            for name in ROUND_CASES}


@contextlib.contextmanager
def switches(env):
    """The SHDPE_* switches of this file set to `env` and no others (the engine reads them at create)."""
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


def run(E, top, att, split, lb=8, grid=None, rnd=None, env=None, sources=None, tune=False, paths=None, devices=None):
    """One engine: the table (or the rows of `sources`), then the paths of
    `paths` = (src, dst); its stats and per-shard batch_info."""
    env = dict(env or {})
    if split is not None:
        env["SHDPE_POST_SPLIT"] = int(split)
    env["SHDPE_BATCH_LB"] = lb
    if grid is not None:
        env["SHDPE_BATCH_GRID"] = grid
    if rnd is not None:
        env["SHDPE_BATCH_ROUND"] = rnd
    with switches(env):
        kw = {} if devices is None else {"devices": devices}
        eng = E.Engine(top, att, force_mode=5, debug_flags=E.DEBUG_ENV | E.DEBUG_COUNTERS, **kw)
    try:
        assert np.array_equal(eng.attached, att)
        r = SimpleNamespace(T=eng.T, lb=lb)
        if tune:
            eng.tune()
            r.tuned = (eng.stats(), eng.post_split_info(), eng.batch_info(0))
        if sources is None:
            eng.compute_all()
            if devices is not None:
                r.shard_rows = eng.get_rows(0, eng.T)       # from the owning shards
                r.bounds = eng.shard_bounds()
                eng.gather()
            rows = eng.get_rows(0, eng.T)
        else:
            eng.compute_rows(sources)
            got = [eng.get_row(int(s)) for s in sources]
            rows = {k: np.stack([g[k] for g in got]) for k in FIELDS}
        r.rows = {k: rows[k] for k in FIELDS}
        r.st = eng.stats()
        r.info = eng.post_split_info()
        r.binfo = [eng.batch_info(i) for i in range(r.st["nShards"])]
        if paths is not None:
            r.paths = eng.get_paths(paths[0], paths[1], hops=True)
            r.pinfo = eng.paths_info()
            r.binfo_after_paths = eng.batch_info(0)
    finally:
        eng.close()
    return r


def ceil_div(a, b):
    return -(-a // b)


def check_rounds(r, nrows, per_round, slots, ctx, shard=0, partial=None):
    """The shard ran ceil(batches / per_round) >= 2 rounds of at most per_round
    batches on `slots` scratch slots, in one relax call over nrows rows."""
    b = r.binfo[shard]
    print(f"{ctx}: batch_info {b}")
    assert b["batches"] == ceil_div(nrows, r.lb), (ctx, b, nrows)
    assert b["slots"] == min(slots, b["batches"]) and b["perRound"] == max(per_round, b["slots"]), (ctx, b)
    assert b["rounds"] == ceil_div(b["batches"], b["perRound"]) and b["rounds"] >= 2, (ctx, b)
    if partial:
        assert b["batches"] % b["perRound"] != 0, (ctx, b)
    return b


def check_one_round(r, nrows, ctx):
    b = r.binfo[0]
    assert b["rounds"] == 1 and b["batches"] == ceil_div(nrows, r.lb) and b["perRound"] >= b["batches"], (ctx, b)


def same_bytes(a, b, ctx):
    for k in FIELDS:
        assert a[k].tobytes() == b[k].tobytes(), (ctx, k)


@pytest.fixture(scope="module")
def one_round(E, expected):
    """The one-round table of (case, lanes, split, further switches): no grid
    and no round cap, computed once and checked against the oracle."""
    cache = {}

    def get(case, lb, split, **env):
        key = (case, lb, bool(split), tuple(sorted(env.items())))
        if key not in cache:
            top, att, _ = CASES[case]
            r = run(E, top, att, split, lb=lb, env=env)
            ctx = f"{case} lb {lb} split {int(split)} {env} one round"
            check_one_round(r, r.T, ctx)
            assert r.info["split"] == int(split), (ctx, r.info)
            check_rows(r.rows, expected[case], ctx)
            cache[key] = r
        return cache[key]
    return get


# ---- (a) rows over many rounds ----------------------------------------------------

@pytest.mark.parametrize("grid,rnd", SETTINGS)
@pytest.mark.parametrize("lb", [8, 16])
@pytest.mark.parametrize("case", ROUND_CASES)
def test_rows_over_many_rounds(E, expected, one_round, case, lb, grid, rnd):
    """Every round after the first starts on the flag words, in-arc hit bits,
    label records and redo list the round before left behind; the last round
    is shorter than the others."""
    top, att, tiefree = CASES[case]
    for split in (True, False):
        ctx = f"{case} lb {lb} grid {grid} round {rnd} split {int(split)}"
        ref = one_round(case, lb, split)
        r = run(E, top, att, split, lb=lb, grid=grid, rnd=rnd)
        check_rounds(r, r.T, rnd, grid, ctx, partial=lb == 8 and (grid, rnd) != (1, 1))
        st = r.st
        assert st["mode"] == 1 and st["batched"] == 1 and st["batchLanes"] == lb and st["launchesSparse"] == 1, (ctx, st)
        assert r.info["split"] == int(split), (ctx, r.info)
        check_rows(r.rows, expected[case], ctx)
        same_bytes(r.rows, ref.rows, ctx)
        assert st["rowsTieRepaired"] == 0, (ctx, st)
        if tiefree:
            assert st["rowsExact"] == 0, (ctx, st)
        else:
            assert st["rowsExact"] == ref.st["rowsExact"], (ctx, st, ref.st)
            assert st["rowsTieEarly"] == ref.st["rowsTieEarly"], (ctx, st, ref.st)
        if tiefree is False:
            assert st["rowsExact"] > 0, (ctx, st)
        if case == "ba1200":
            assert r.info["redoBatches"] == 0, (ctx, r.info)


# ---- (b) predecessor filter across rounds -----------------------------------------

@pytest.mark.parametrize("case", ["ba1200", "directed"])
def test_pred_filter_across_rounds(E, expected, one_round, case):
    """A round's in-arc hit bits are those of its own relax: with the filter
    the predecessor pass gathers fewer in-arcs and writes the same rows.  (The
    counters are not compared between runs: the relax's atomics make the set
    of flagged arcs run-dependent.)"""
    top, att, _ = CASES[case]
    for split in (True, False):
        got = {}
        for filt in (0, 1):
            ctx = f"{case} split {int(split)} filter {filt}"
            r = run(E, top, att, split, grid=2, rnd=3, env={"SHDPE_PRED_FILTER": filt})
            check_rounds(r, r.T, 3, 2, ctx, partial=True)
            assert r.info["split"] == int(split), (ctx, r.info)
            check_rows(r.rows, expected[case], ctx)
            same_bytes(r.rows, one_round(case, 8, split).rows, ctx)
            assert r.st["rowsExact"] == 0 and r.st["rowsTieRepaired"] == 0, (ctx, r.st)
            claimed, gathered = r.st["predArcsClaimed"], r.st["predArcsGathered"]
            print(f"{ctx}: in-arcs claimed {claimed} gathered {gathered}")
            if filt:
                assert 0 < gathered <= claimed, (ctx, r.st)
                if case == "ba1200":
                    assert gathered < claimed, (ctx, r.st)
            else:
                assert 0 < gathered == claimed, (ctx, r.st)     # every in-arc of every claimed entry
            got[filt] = r.rows
        same_bytes(got[0], got[1], f"{case} split {int(split)}")


# ---- (c) the redo launch in every round -------------------------------------------

def test_redo_launch_in_every_round(E, oracle_mod):
    """A chain of 2,400 vertices is deeper than the label part's walk budget:
    every batch of every round goes onto the redo list (round-relative batch
    numbers, its counter zeroed per round, its total kept) and the one post
    kernel's second attempt writes the rows."""
    n = 2400
    top = chain(n, seed=n)
    att = np.arange(n, dtype=np.int32)
    srcs = np.arange(17, n, 60, dtype=np.int32)
    assert srcs.shape[0] == 40
    exp = oracle_mod.OracleGraph(top).rows(srcs, att, threads=8)
    got = {}
    for split in (True, False):
        ctx = f"chain split {int(split)}"
        r = run(E, top, att, split, grid=1, rnd=2, sources=srcs)
        b = check_rounds(r, srcs.shape[0], 2, 1, ctx, partial=True)
        assert b["batches"] == 5 and b["rounds"] == 3, b
        check_rows(r.rows, exp, ctx)
        assert r.st["rowsExact"] == 0, (ctx, r.st)
        assert r.info["split"] == int(split), (ctx, r.info)
        assert r.info["redoBatches"] == (b["batches"] if split else 0), (ctx, r.info)
        got[split] = r.rows
    same_bytes(got[True], got[False], "chain")


# ---- (d) tie export across rounds --------------------------------------------------

@pytest.mark.parametrize("split", [True, False])
def test_tie_export_across_rounds(E, expected, one_round, split):
    """k_tie_export serves a round's requests only (the round word), on slots
    whose counter runs on from round to round.  SHDPE_TIE_CORRUPT=3: slot 0's
    row is treated as violated and takes the full emulation."""
    top, att, _ = CASES["ties"]
    ref = one_round("ties", 8, split)
    assert ref.st["rowsTieEarly"] > 0, ref.st
    r = run(E, top, att, split, grid=2, rnd=3)
    ctx = f"ties split {int(split)}"
    check_rounds(r, r.T, 3, 2, ctx, partial=True)
    assert r.info["split"] == int(split), (ctx, r.info)
    check_rows(r.rows, expected["ties"], ctx)
    same_bytes(r.rows, ref.rows, ctx)
    assert r.st["rowsTieEarly"] == ref.st["rowsTieEarly"] and r.st["rowsExact"] == ref.st["rowsExact"], (r.st, ref.st)
    assert r.st["rowsTieRepaired"] == 0, r.st
    c = run(E, top, att, split, grid=2, rnd=3, env={"SHDPE_TIE_CORRUPT": 3})
    check_rounds(c, c.T, 3, 2, ctx + " corrupt", partial=True)
    check_rows(c.rows, expected["ties"], ctx + " corrupt")
    assert c.st["rowsExact"] == ref.st["rowsExact"], (c.st, ref.st)
    assert c.st["rowsTieEarly"] == ref.st["rowsTieEarly"] - 1, (c.st, ref.st)


# ---- (e) the tie slots run out in an early round -----------------------------------

@pytest.mark.parametrize("split", [True, False])
def test_tie_slots_run_out_in_an_early_round(E, expected, one_round, split):
    """Three tie slots: the first rounds' tie rows take them, the tie rows of
    every later round go to the full emulation.  compute_all is one relax call
    on this table (launchesSparse == 1) and the slot counter is zeroed per
    call, not per round: at most 3 early-stop rows."""
    top, att, _ = CASES["ties"]
    ref = one_round("ties", 8, split)
    r = run(E, top, att, split, grid=2, rnd=3, env={"SHDPE_TIE_SLOTS": 3})
    ctx = f"ties 3 slots split {int(split)}"
    check_rounds(r, r.T, 3, 2, ctx, partial=True)
    assert r.info["split"] == int(split), (ctx, r.info)
    check_rows(r.rows, expected["ties"], ctx)
    for k in ("lat", "rel", "hops", "pred"):
        assert r.rows[k].tobytes() == ref.rows[k].tobytes(), (ctx, k)
    assert r.st["launchesSparse"] == 1, r.st
    assert r.st["rowsExact"] == ref.st["rowsExact"], (r.st, ref.st)
    assert 0 < r.st["rowsTieEarly"] < ref.st["rowsTieEarly"], (r.st, ref.st)
    assert r.st["rowsTieEarly"] <= 3 * r.st["launchesSparse"], r.st
    assert r.st["rowsTieRepaired"] == 0, r.st


# ---- (f) no tie slots ---------------------------------------------------------------

@pytest.mark.parametrize("rounds", ["one", "many"])
@pytest.mark.parametrize("case", ["ties", "ba1200"])
def test_no_tie_slots(E, expected, one_round, case, rounds):
    """SHDPE_TIE_SLOTS=0 is the shard past 2^30 arcs: no deferred buffer, so
    the label part hands every tie batch to the redo launch and the tie rows
    come out of the full emulation; without ties nothing takes the redo launch."""
    top, att, tiefree = CASES[case]
    got = {}
    for split in (True, False):
        ref = one_round(case, 8, split)
        ctx = f"{case} no slots {rounds} split {int(split)}"
        kw = {"grid": 2, "rnd": 3} if rounds == "many" else {}
        r = run(E, top, att, split, env={"SHDPE_TIE_SLOTS": 0}, **kw)
        if rounds == "many":
            check_rounds(r, r.T, 3, 2, ctx, partial=True)
        else:
            check_one_round(r, r.T, ctx)
        assert r.info["split"] == int(split), (ctx, r.info)
        check_rows(r.rows, expected[case], ctx)
        for k in ("lat", "rel", "hops", "pred"):
            assert r.rows[k].tobytes() == ref.rows[k].tobytes(), (ctx, k)
        assert r.st["rowsTieEarly"] == 0 and r.st["rowsTieRepaired"] == 0, (ctx, r.st)   # zero slots: none early
        assert r.st["rowsExact"] == ref.st["rowsExact"], (ctx, r.st, ref.st)
        if tiefree:
            assert r.st["rowsExact"] == 0 and r.info["redoBatches"] == 0, (ctx, r.st, r.info)
        else:
            assert ref.st["rowsTieEarly"] > 0 and r.st["rowsExact"] > 0, (ctx, r.st, ref.st)
            assert (r.info["redoBatches"] > 0) == split, (ctx, r.info)
        got[split] = r.rows
    same_bytes(got[True], got[False], f"{case} {rounds}")


# ---- tie slots filled in line, beside the requests of an earlier call ----------------------

DEEP_K, FLAT_K = 2400, 80
DEEP_SRC = np.concatenate([np.arange(3, 283, 35), DEEP_K + np.arange(2396, 2116, -35)]).astype(np.int32)
FLAT_SRC = (2 * DEEP_K + np.arange(2, 2 * FLAT_K, 10)).astype(np.int32)


def _two_ladders():
    """A ladder of 2 x 2,400 vertices and, unconnected to it, one of 2 x 80."""
    a, b = ladder(DEEP_K, seed=DEEP_K), ladder(FLAT_K, seed=FLAT_K)
    return Topology(a.n + b.n, False, np.concatenate([a.src, b.src + a.n]), np.concatenate([a.dst, b.dst + a.n]),
                    np.concatenate([a.latency, b.latency]), np.concatenate([a.loss, b.loss]), None)


@pytest.mark.parametrize("rounds", ["one", "many"])
def test_tie_slots_filled_in_line_have_no_request(E, oracle_mod, rounds):
    """Every row of a ladder is a tie row.  In the small ladder the post
    kernel (or its label part) defers the export: the slots get requests of
    round 0, 1, ... for k_tie_export.  The trees of the large one are deeper
    than the walk budget: the batches take the post kernel's second attempt
    (the redo launch, when it is split), which fills the slots in line and
    writes no request.  k_tie_export must not serve what those slots' request
    words held before -- the first call's requests, or whatever the allocator
    left -- or a slot ends up with another row's distances and parents
    (before the requests were cleared per call: rows repaired by the exact
    kernel's cross-check, and wrong reliabilities where it did not notice)."""
    assert DEEP_SRC.shape[0] == 16 and FLAT_SRC.shape[0] == 16
    top = _two_ladders()
    att = np.arange(top.n, dtype=np.int32)
    og = oracle_mod.OracleGraph(top)
    exp = {"flat": og.rows(FLAT_SRC, att, threads=8), "deep": og.rows(DEEP_SRC, att, threads=8)}
    got = {}
    for split in (True, False):
        env = {"SHDPE_POST_SPLIT": int(split), "SHDPE_BATCH_LB": 8}
        if rounds == "many":
            env.update(SHDPE_BATCH_GRID=1, SHDPE_BATCH_ROUND=1)
        with switches(env):
            eng = E.Engine(top, att, force_mode=5, debug_flags=E.DEBUG_ENV | E.DEBUG_COUNTERS)
        try:
            # (the third call: deferred requests again, after the slots were filled in line)
            calls = (("flat", FLAT_SRC, exp["flat"]), ("deep", DEEP_SRC, exp["deep"]),
                     ("flat again", FLAT_SRC[::-1].copy(), {k: v[::-1] for k, v in exp["flat"].items()}))
            for name, srcs, want in calls:
                ctx = f"ladders {rounds} split {int(split)} {name}"
                eng.reset_stats()
                eng.compute_rows(srcs)
                rows = [eng.get_row(int(s)) for s in srcs]
                rows = {k: np.stack([g[k] for g in rows]) for k in FIELDS}
                st, info, b = eng.stats(), eng.post_split_info(), eng.batch_info(0)
                print(f"{ctx}: {b} early {st['rowsTieEarly']} exact {st['rowsExact']} repaired "
                      f"{st['rowsTieRepaired']} redo {info['redoBatches']}")
                assert b["batches"] == 2 and b["rounds"] == (2 if rounds == "many" else 1), (ctx, b)
                assert info["split"] == int(split), (ctx, info)
                # (the second attempt is visible as the redo launch; the one post kernel runs it inside)
                if split:
                    assert (info["redoBatches"] > 0) == (name == "deep"), (ctx, info)
                check_rows(rows, want, ctx)
                # every row is a tie row with a slot of its own, and no slot held another row's distances
                assert st["rowsExact"] == 16 and st["rowsTieEarly"] == 16, (ctx, st)
                assert st["rowsTieRepaired"] == 0, (ctx, st)
                got[(split, name)] = rows
        finally:
            eng.close()
    for name in ("flat", "deep", "flat again"):
        same_bytes(got[(True, name)], got[(False, name)], f"ladders {rounds} {name}")


# ---- (g) shd_pe_get_paths over rounds ------------------------------------------------

@pytest.mark.parametrize("case", ["directed", "ties"])
def test_get_paths_over_rounds(E, case):
    """The batch tier's pass walks each round's requests (base r0 * lanes) on
    the round's distance arrays before the next relax overwrites them."""
    top, att, _ = CASES[case]
    rng = np.random.default_rng(5)
    src = rng.choice(att, 200).astype(np.int32)
    dst = rng.choice(att, 200).astype(np.int32)
    for split in (True, False):
        ctx = f"{case} paths split {int(split)}"
        ref = run(E, top, att, split, paths=(src, dst))
        check_one_round(ref, ref.T, ctx)
        r = run(E, top, att, split, grid=2, rnd=3, paths=(src, dst))
        b = check_rounds(r, r.T, 3, 2, ctx, partial=True)
        assert r.info["split"] == int(split), (ctx, r.info)
        # the paths' pass runs the same loop (3 batches a round) over more sources than a round holds,
        # and is not counted among the table's rounds
        assert np.unique(src).shape[0] > 2 * b["perRound"] * r.lb
        assert r.binfo_after_paths == b, (ctx, r.binfo_after_paths, b)
        for name, x, y in zip(("offsets", "verts", "status", "hop lat", "hop rel"), r.paths, ref.paths):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), (ctx, name)
        assert (np.asarray(r.paths[2]) == 0).sum() > 100, ctx          # real paths were compared
        print(f"{ctx}: paths_info {r.pinfo} one round {ref.pinfo}")
        assert r.pinfo["batch"] > 0, (ctx, r.pinfo)
        if case == "ties":
            assert r.pinfo["tie"] > 0, (ctx, r.pinfo)
        for k in ("batch", "tie", "emulated"):
            assert r.pinfo[k] == ref.pinfo[k], (ctx, k, r.pinfo, ref.pinfo)


# ---- (h) tune over rounds --------------------------------------------------------------

@pytest.mark.parametrize("fail", [0, 6])
def test_tune_over_rounds(E, expected, fail):
    """shd_pe_tune's trials sum their per-round event times; the compute after
    it runs the rounds of the lanes it kept, and its own computes are not
    counted.  SHDPE_TUNE_FAIL_WPE=6: that variant is not picked."""
    top, att, _ = CASES["ba1200"]
    env = {"SHDPE_TUNE_FAIL_WPE": fail} if fail else {}
    r = run(E, top, att, None if not fail else True, lb=16, grid=2, rnd=3, env=env, tune=True)
    st, info, b0 = r.tuned
    ctx = f"tune fail {fail}"
    print(f"{ctx}: split {info['split']} label waves {info['labelWaves']} waves {st['batchWaves']} / {st['batchPostWaves']}")
    assert b0["rounds"] == 0 and b0["batches"] == 0 and b0["perRound"] == 3 and b0["slots"] == 2, (ctx, b0)
    assert info["labelWaves"] in ((4, 6, 8) if info["split"] else (0,)), (ctx, info)
    if fail:
        assert info["split"] == 1 and info["labelWaves"] != fail, (ctx, info)
        assert st["batchWaves"] != fail and st["batchPostWaves"] != fail, (ctx, st)
    r.lb = r.st["batchLanes"]                                   # the lanes the tune kept
    assert r.lb == 16, r.st
    check_rounds(r, r.T, 3, 2, ctx)
    assert r.info == dict(info, redoBatches=r.info["redoBatches"]), (ctx, r.info, info)
    check_rows(r.rows, expected["ba1200"], ctx)
    assert r.st["rowsExact"] == 0 and r.st["rowsTieRepaired"] == 0, (ctx, r.st)


# ---- (i) two shards ---------------------------------------------------------------------

def test_two_shards_report_their_own_rounds(E, expected, one_round):
    top, att, _ = CASES["ba1200"]
    for split in (True, False):
        ctx = f"two shards split {int(split)}"
        r = run(E, top, att, split, grid=2, rnd=3, devices=[0, 0])
        assert r.st["nShards"] == 2 and len(r.binfo) == 2 and r.st["rowsComputed"] == r.T, (ctx, r.st)
        bounds = [int(x) for x in r.bounds]
        assert bounds[0] == 0 and bounds[2] == r.T and 0 < bounds[1] < r.T, bounds
        for i in range(2):
            check_rounds(r, bounds[i + 1] - bounds[i], 3, 2, f"{ctx} shard {i}", shard=i)
        assert sum(b["batches"] for b in r.binfo) >= ceil_div(r.T, r.lb)
        assert r.info["split"] == int(split), (ctx, r.info)
        check_rows(r.rows, expected["ba1200"], ctx + " gathered")
        same_bytes(r.rows, one_round("ba1200", 8, split).rows, ctx + " gathered")
        same_bytes(r.shard_rows, r.rows, ctx + " per shard")
        assert r.st["rowsExact"] == 0 and r.st["rowsTieRepaired"] == 0, (ctx, r.st)
