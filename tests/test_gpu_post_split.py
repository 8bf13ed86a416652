"""The batched post kernel as two kernels (predecessor part, label part;
SHDPE_POST_SPLIT=1) and as one (=0) compute the same table, bit-exact against
the oracle, at 8 and 16 lanes and in the 4-, 6- and 8-wave variants; batches
the label part cannot finish (trees deeper than the walk budget) take the
redo launch; several batches per workgroup; shd_pe_get_paths; shd_pe_tune.

Graphs and row comparison: tests/post_split_cases.py."""
import numpy as np
import pytest

from post_split_cases import CASES, FIELDS, check_rows
from post_split_cases import chain as _chain
from shdpe.graph import Topology

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    from shdpe import engine
    engine.load_library()
    return engine


@pytest.fixture(scope="module")
def expected(oracle_mod):
    """The oracle's rows of every case, computed once."""
    return {name: oracle_mod.OracleGraph(top).rows(att, att, threads=8) for name, (top, att, _) in CASES.items()}


def table(E, top, att, split, monkeypatch, env=(), sources=None, tune=False):
    monkeypatch.setenv("SHDPE_POST_SPLIT", "1" if split else "0")
    for k, v in env:
        monkeypatch.setenv(k, str(v))
    eng = E.Engine(top, att, force_mode=5, debug_flags=E.DEBUG_ENV | E.DEBUG_COUNTERS)
    assert np.array_equal(eng.attached, att)
    if tune:
        eng.tune()
    if sources is None:
        eng.compute_all()
        rows = eng.get_rows(0, eng.T)
    else:
        eng.compute_rows(sources)
        got = [eng.get_row(int(s)) for s in sources]
        rows = {k: np.stack([g[k] for g in got]) for k in FIELDS}
    st = eng.stats()
    info = dict(eng.post_split_info(), **eng.batch_info())     # + perRound, slots, rounds, batches
    eng.close()
    return {k: rows[k] for k in FIELDS}, st, info


@pytest.mark.parametrize("wpe", [4, 6, 8])
@pytest.mark.parametrize("lb", [8, 16])
@pytest.mark.parametrize("case", list(CASES))
def test_rows_exact_split_and_unsplit(E, expected, monkeypatch, case, lb, wpe):
    top, att, tiefree = CASES[case]
    exp = expected[case]
    got = {}
    for split in (True, False):
        rows, st, info = table(E, top, att, split, monkeypatch,
                               env=(("SHDPE_BATCH_LB", lb), ("SHDPE_BATCH_WPE", wpe)))
        got[split] = rows
        ctx = f"{case} lb {lb} wpe {wpe} split {int(split)}"
        assert st["mode"] == 1 and st["batched"] == 1 and st["batchLanes"] == lb, (ctx, st)
        assert st["batchWaves"] == wpe and st["batchPostWaves"] == wpe, (ctx, st)
        # a switch that is silently off cannot pass
        assert info["split"] == int(split) and info["labelWaves"] == (wpe if split else 0), (ctx, info)
        check_rows(rows, exp, ctx)
        assert st["rowsTieRepaired"] == 0, (ctx, st)
        if tiefree:
            assert st["rowsExact"] == 0, (ctx, st)
        elif tiefree is False:
            assert st["rowsExact"] > 0, (ctx, st)       # tie rows: the export and the exact kernel
        claimed, gathered = st["predArcsClaimed"], st["predArcsGathered"]
        print(f"{ctx}: in-arcs claimed {claimed} gathered {gathered} redo {info['redoBatches']}")
        assert 0 < gathered <= claimed, (ctx, st)
        if case == "ba1200":
            assert gathered < claimed, (ctx, st)        # the counters moved with the predecessor part
            assert info["redoBatches"] == 0, (ctx, info)   # shallow, tie-free: nothing to redo
    for k in FIELDS:
        assert got[True][k].tobytes() == got[False][k].tobytes(), (case, lb, wpe, k)


@pytest.fixture(scope="module")
def chain_case(oracle_mod):
    """The 2,400-vertex chain of test_deep_tree_takes_the_redo_launch, its
    sources and the oracle's rows of them, computed once."""
    n = 2400
    top = _chain(n, seed=n)
    att = np.arange(n, dtype=np.int32)
    srcs = np.array([0, n - 1, n // 2, n // 3, 7], np.int32)
    return top, att, srcs, oracle_mod.OracleGraph(top).rows(srcs, att, threads=8), True


@pytest.mark.parametrize("wpe", [4, 8])
@pytest.mark.parametrize("lb", [8, 16])
@pytest.mark.parametrize("case", ["ba1200", "ties", "chain"])
def test_rows_exact_one_kernel(E, chain_case, expected, monkeypatch, case, lb, wpe):
    """SHDPE_BATCH_SPLIT=0: the whole batch in one kernel (relax, full
    predecessor pass, labels, rows, in-line tie export) computes the table of
    the split kernels, bit-exact against the oracle.  The chain is deeper than
    WALK_BUDGET: the kernel's own sweeps and second writer pass write its rows.
    (The engine offers the 6-wave variant only to the split kernels.)"""
    if case == "chain":
        top, att, srcs, exp, tiefree = chain_case
    else:
        (top, att, tiefree), srcs, exp = CASES[case], None, expected[case]
    knobs = (("SHDPE_BATCH_LB", lb), ("SHDPE_BATCH_WPE", wpe))
    ref, _, rinfo = table(E, top, att, True, monkeypatch, env=knobs, sources=srcs)
    assert rinfo["split"] == 1, rinfo
    rows, st, info = table(E, top, att, False, monkeypatch, env=knobs + (("SHDPE_BATCH_SPLIT", 0),), sources=srcs)
    ctx = f"{case} lb {lb} wpe {wpe} one kernel"
    assert st["mode"] == 1 and st["batched"] == 1 and st["batchLanes"] == lb and st["batchWaves"] == wpe, (ctx, st)
    # the one-kernel route ran: no post kernel in the plan, no round of the split kernels
    assert info["split"] == 0 and info["labelWaves"] == 0 and info["redoBatches"] == 0, (ctx, info)
    assert st["batchPostWaves"] == 0, (ctx, st)
    assert info["rounds"] == 0 and info["batches"] == 0, (ctx, info)
    check_rows(rows, exp, ctx)
    assert st["rowsTieRepaired"] == 0, (ctx, st)
    if tiefree:
        assert st["rowsExact"] == 0, (ctx, st)
    else:
        assert st["rowsExact"] > 0, (ctx, st)       # tie rows: the in-line export and the exact kernel
    for k in FIELDS:
        assert np.asarray(rows[k]).tobytes() == np.asarray(ref[k]).tobytes(), (ctx, k)


@pytest.mark.parametrize("lb", [8, 16])
def test_deep_tree_takes_the_redo_launch(E, oracle_mod, monkeypatch, lb):
    """A chain of 2,400 vertices is deeper than WALK_BUDGET (2,048): the label
    part hands the batch back, the one post kernel's second attempt (full
    pass, sweeps) writes its rows; no row goes to the exact kernel."""
    n = 2400
    top = _chain(n, seed=n)
    att = np.arange(n, dtype=np.int32)
    srcs = np.array([0, n - 1, n // 2, n // 3, 7], np.int32)
    exp = oracle_mod.OracleGraph(top).rows(srcs, att, threads=8)
    got = {}
    for split in (True, False):
        rows, st, info = table(E, top, att, split, monkeypatch, env=(("SHDPE_BATCH_LB", lb),), sources=srcs)
        got[split] = rows
        ctx = f"chain lb {lb} split {int(split)}"
        check_rows(rows, exp, ctx)
        assert st["rowsExact"] == 0, (ctx, st)
        assert info["split"] == int(split), (ctx, info)
        assert (info["redoBatches"] > 0) == split, (ctx, info)
    for k in FIELDS:
        assert got[True][k].tobytes() == got[False][k].tobytes(), (lb, k)


@pytest.mark.parametrize("grid", [1, 2])
def test_several_batches_per_workgroup(E, expected, monkeypatch, grid):
    """ba1200's 300 rows are 38 batches of 8: with a grid of 1 or 2 every
    workgroup takes many batches in each kernel, and re-derives its state per
    batch.  (One round; several rounds: tests/test_gpu_rounds.py.)"""
    top, att, _ = CASES["ba1200"]
    rows, st, info = table(E, top, att, True, monkeypatch, env=(("SHDPE_BATCH_LB", 8), ("SHDPE_BATCH_GRID", grid)))
    assert info["split"] == 1 and info["redoBatches"] == 0, info
    check_rows(rows, expected["ba1200"], f"grid {grid}")
    assert st["rowsExact"] == 0, st


@pytest.mark.parametrize("n", [650_000, 660_000])
def test_bitmaps_at_the_lds_edge(E, oracle_mod, monkeypatch, n):
    """The graphs of tests/test_gpu_parity.py's test_large_graph_batched_kernel
    on both sides of the LDS / global bitmap switch, the two parts forced: at
    650,000 vertices the predecessor part's bitmaps take 159 of the CU's 160
    KB, and its heavy list must leave room for the kernel's static shared
    arrays (a dynamic size that fills the LDS is not launchable); at 660,000
    the bitmaps are global and the label part runs its one instantiation."""
    rng = np.random.default_rng(n)
    perm = rng.permutation(n)
    extra = rng.integers(0, n, size=(n, 2))
    src = np.concatenate([perm[:-1], extra[:, 0]])
    dst = np.concatenate([perm[1:], extra[:, 1]])
    key = np.minimum(src, dst).astype(np.int64) * n + np.maximum(src, dst)
    _, first = np.unique(key, return_index=True)
    keep = np.zeros(src.shape[0], bool)
    keep[first] = True
    keep &= src != dst
    src, dst = src[keep], dst[keep]
    top = Topology(n, False, src, dst, rng.uniform(1.0, 50.0, src.shape[0]), rng.uniform(0.0, 0.02, src.shape[0]))
    att = np.array([0, n // 3, n // 2, n - 1], np.int32)
    exp = oracle_mod.OracleGraph(top).rows(att, att, threads=8)
    rows, st, info = table(E, top, att, True, monkeypatch)
    assert info["split"] == 1 and st["batched"] == 1, (info, st)
    check_rows(rows, exp, f"n {n}")


def test_untuned_engine_runs_one_post_kernel(E, expected, monkeypatch):
    """Without a tune and without SHDPE_POST_SPLIT the post kernel is one."""
    top, att, _ = CASES["ba1200"]
    monkeypatch.delenv("SHDPE_POST_SPLIT", raising=False)
    eng = E.Engine(top, att, force_mode=5, debug_flags=E.DEBUG_ENV)
    eng.compute_all()
    info = eng.post_split_info()
    rows = eng.get_rows(0, eng.T)
    eng.close()
    assert info == {"split": 0, "labelWaves": 0, "redoBatches": 0}, info
    check_rows(rows, expected["ba1200"], "untuned")


@pytest.mark.parametrize("lb", [8, 16])
def test_get_paths_same_under_both_settings(E, monkeypatch, lb):
    """shd_pe_get_paths' pass (the one post kernel without its row stores)
    shares the rounds with the split launches: the same paths."""
    top, att, _ = CASES["directed"]
    rng = np.random.default_rng(5)
    src = rng.choice(att, 200).astype(np.int32)
    dst = rng.choice(att, 200).astype(np.int32)
    out = {}
    for split in (True, False):
        monkeypatch.setenv("SHDPE_BATCH_LB", str(lb))
        monkeypatch.setenv("SHDPE_POST_SPLIT", "1" if split else "0")
        eng = E.Engine(top, att, force_mode=5, debug_flags=E.DEBUG_ENV)
        eng.compute_all()                       # (the split launches first, then the paths' pass)
        out[split] = eng.get_paths(src, dst)
        assert eng.post_split_info()["split"] == int(split)
        eng.close()
    for a, b in zip(out[True], out[False]):
        assert np.array_equal(a, b)
    offsets, verts, status = out[True]
    assert (np.asarray(status) == 0).sum() > 100          # real paths were compared


def test_tune_keeps_rows_exact(E, expected, monkeypatch):
    top, att, _ = CASES["ba1200"]
    monkeypatch.delenv("SHDPE_POST_SPLIT", raising=False)
    monkeypatch.setenv("SHDPE_BATCH_LB", "16")
    eng = E.Engine(top, att, force_mode=5, debug_flags=E.DEBUG_ENV)
    eng.tune()
    info = eng.post_split_info()
    st = eng.stats()
    print(f"tune: split {info['split']} label waves {info['labelWaves']} post waves {st['batchPostWaves']}")
    assert info["labelWaves"] in ((4, 6, 8) if info["split"] else (0,)), info
    eng.compute_all()
    rows = eng.get_rows(0, eng.T)
    assert eng.stats()["rowsExact"] == 0
    eng.close()
    check_rows(rows, expected["ba1200"], "tuned")


@pytest.mark.parametrize("wpe", [4, 6, 8])
def test_tune_label_pick_is_never_the_failing_variant(E, expected, monkeypatch, wpe):
    """SHDPE_TUNE_FAIL_WPE: the relax of that wave count fails every batch, so
    the variant is excluded from every pick, the label part's included (with
    the split forced, so that there is a label pick)."""
    top, att, _ = CASES["ba1200"]
    monkeypatch.setenv("SHDPE_TUNE_FAIL_WPE", str(wpe))
    monkeypatch.setenv("SHDPE_BATCH_LB", "16")
    monkeypatch.setenv("SHDPE_POST_SPLIT", "1")
    eng = E.Engine(top, att, force_mode=5, debug_flags=E.DEBUG_ENV)
    eng.tune()
    info = eng.post_split_info()
    st = eng.stats()
    assert info["split"] == 1 and info["labelWaves"] in (4, 6, 8) and info["labelWaves"] != wpe, info
    assert st["batchWaves"] != wpe and st["batchPostWaves"] != wpe, st
    eng.compute_all()
    rows = eng.get_rows(0, eng.T)
    assert eng.stats()["rowsExact"] == 0
    eng.close()
    check_rows(rows, expected["ba1200"], f"fail {wpe}")
