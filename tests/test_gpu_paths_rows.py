"""GPU tests of the path extraction's row tier (shd_pe_paths_set_row_tier): the
per-row sparse kernel's parents and the dense min-plus distances walked instead
of one full emulation per source.  Every path against the oracle's igraph
Dijkstra, the bytes against the emulation-only call, the per-tier counters,
grouping / chunking, the switches, sharding and the absence of side effects."""
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN
from shdpe import generators as G
from shdpe.graph import Topology
from test_gpu_paths import CASES as BASE_CASES
from test_gpu_paths import E, _Oracle, _check_against_oracle, _requests  # noqa: F401  (E: the fixture)

pytestmark = pytest.mark.gpu

ALL = "all"
CASES = {
    # name: (graph, attached (None: every third vertex), forceMode, fold check, dense)
    "sparse_tiefree": (lambda: G.random_sparse(800, 5, seed=34), None, 0, True, False),
    "sparse_quantized": (lambda: G.random_sparse(800, 5, seed=32, quantum=0.5), None, 0, False, False),
    "sparse_directed": (lambda: G.random_sparse(700, 5, seed=31, directed=True), None, 0, False, False),
    "sparse_vloss": (lambda: G.random_sparse(600, 5, seed=35, vloss=True), None, 0, False, False),
    "dense": (lambda: G.dense(300, seed=3, drop_edge=True), None, 4, False, True),
    "dense_quantized": (lambda: G.dense(300, seed=3, drop_edge=True, quantum=2.0), ALL, 4, False, True),
    "directed_forced_dense": (lambda: G.random_sparse(700, 5, seed=31, directed=True), None, 4, False, True),
}
TIE_FREE = ("sparse_tiefree", "dense", "directed_forced_dense")


@functools.lru_cache(maxsize=None)
def _case(name):
    make, att, force, fold, dense = CASES[name]
    top = make()
    att = np.arange(top.n, dtype=np.int32) if att is ALL else np.arange(0, top.n, 3, dtype=np.int32)
    return top, att, force, fold, dense


def _engine(E, name, row_tier=True, **kw):
    top, att, force, _, dense = _case(name)
    eng = E.Engine(top, att, force_mode=force, **kw)
    st = eng.stats()
    assert st["mode"] == 3 if dense else st["batched"] == 0 and st["mode"] == 1
    if row_tier:
        eng.set_paths_row_tier(True)
    return eng


def _n_uniq(src, dst):
    return np.unique(src[src != dst]).shape[0]


def _same_bytes(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


# ---- 1. against the oracle ------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_rows_match_oracle(E, oracle_mod, name):
    """Path, length = hops + 1, hop attributes bit for bit, fold where tie-free."""
    top, att, _, fold, _ = _case(name)
    eng = _engine(E, name)
    orc = _Oracle(oracle_mod, top, eng.attached)
    src, dst = _requests(att)
    _check_against_oracle(E, eng, orc, src, dst, fold)
    info = eng.paths_info()
    eng.close()
    print(name, info)
    assert info["batch"] == 0 and info["rows"] > 0
    assert info["rows"] + info["tie"] + info["emulated"] == _n_uniq(src, dst)    # each unique source in one tier


# ---- 2. the tiers agree ---------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_tiers_agree(E, name):
    """Every row's requests: the row tier's bytes are those of a fresh engine
    that never switched it on (the grouped emulation alone)."""
    _, att, _, _, _ = _case(name)
    src, dst = _requests(att, n_src=att.shape[0], n_dst=3)
    n_uniq = _n_uniq(src, dst)
    eng = _engine(E, name)
    fast = eng.get_paths(src, dst, hops=True)
    info = eng.paths_info()
    eng.close()
    eng = _engine(E, name, row_tier=False)
    slow = eng.get_paths(src, dst, hops=True)
    slow_info = eng.paths_info()
    eng.close()
    print(name, n_uniq, info)
    assert slow_info["rows"] == 0 and slow_info["emulated"] == n_uniq
    _same_bytes(fast, slow)
    assert info["batch"] == 0
    assert info["batch"] + info["tie"] + info["emulated"] + info["rows"] == n_uniq
    if name in TIE_FREE:
        assert info["rows"] == n_uniq
        assert info["emulated"] == info["tie"] == info["groups"] == info["handed_on"] == 0
    if name == "sparse_quantized":
        # from the oracle's distances and the predecessor rule: 14 of the 267 rows hold a tied vertex
        assert n_uniq == 267
        assert info["rows"] + info["tie"] + info["emulated"] == n_uniq
        assert 1 <= info["tie"] + info["emulated"] <= n_uniq // 4
        assert info["rows"] >= n_uniq // 2
    if name == "dense_quantized":
        # the same rule along each requested chain: 13 of the 821 walking requests meet a tie,
        # from 12 of the 300 sources; at most 10% of the requests may be handed on
        assert n_uniq == 300
        assert 1 <= info["handed_on"] <= 82
        assert info["emulated"] >= 1 and info["rows"] >= 250
        assert info["rows"] + info["emulated"] == n_uniq


@pytest.mark.parametrize("var,val", [("SHDPE_TIE_SLOTS", "0"), ("SHDPE_TIE_CORRUPT", "1")])
def test_sparse_tie_rows_without_a_good_slot(E, monkeypatch, var, val):
    """Tie rows that get no slot (SHDPE_TIE_SLOTS=0) stay in the work set with
    all their requests; a slot whose distances are not its row's
    (SHDPE_TIE_CORRUPT) fails the consistency check and is handed on.  Either
    way the grouped emulation finishes them with the same bytes."""
    name = "sparse_quantized"
    _, att, _, _, _ = _case(name)
    src, dst = _requests(att, n_src=att.shape[0], n_dst=3)
    n_uniq = _n_uniq(src, dst)
    eng = _engine(E, name)
    ref = eng.get_paths(src, dst, hops=True)
    ref_info = eng.paths_info()
    eng.close()
    monkeypatch.setenv(var, val)
    eng = _engine(E, name, debug_flags=E.DEBUG_ENV)
    got = eng.get_paths(src, dst, hops=True)
    info = eng.paths_info()
    eng.close()
    print(var, ref_info, info)
    _same_bytes(got, ref)
    assert info["rows"] + info["tie"] + info["emulated"] == n_uniq
    assert info["rows"] == ref_info["rows"]
    assert info["emulated"] > ref_info["emulated"] and info["tie"] < ref_info["tie"]
    if var == "SHDPE_TIE_SLOTS":
        assert info["tie"] == 0 and info["handed_on"] == ref_info["handed_on"]
    else:
        assert info["handed_on"] > ref_info["handed_on"]


# ---- 3. groups and chunks -------------------------------------------------------

def test_sparse_groups_and_chunks(E, monkeypatch):
    """600 unique sources in row-tier groups of 64 and staging chunks of 100
    requests (scratch slots and group indices reused): the unchunked bytes."""
    top = G.random_sparse(800, 5, seed=34)
    att = np.arange(800, dtype=np.int32)
    rng = np.random.default_rng(9)
    src = rng.permutation(att)[:600].astype(np.int32)
    dst = rng.choice(att, 600).astype(np.int32)
    assert _n_uniq(src, dst) == 600
    eng = E.Engine(top, att)
    eng.set_paths_row_tier(True)
    ref = eng.get_paths(src, dst, hops=True)
    ref_info = eng.paths_info()
    eng.close()
    monkeypatch.setenv("SHDPE_PATHS_GROUP", "64")
    monkeypatch.setenv("SHDPE_PATHS_CHUNK", "100")
    eng = E.Engine(top, att, debug_flags=E.DEBUG_ENV)
    eng.set_paths_row_tier(True)
    got = eng.get_paths(src, dst, hops=True)
    info = eng.paths_info()
    eng.close()
    _same_bytes(got, ref)
    assert ref_info["rows"] == 600 and info["rows"] == 600
    assert info["emulated"] == info["groups"] == 0


@pytest.mark.parametrize("paths_chunk", [None, "100"])
def test_dense_chunks(E, monkeypatch, paths_chunk):
    """300 sources in dense chunks of 64 rows (five, the last partial; row
    indices of D reused), alone and under staging chunks of 100 requests."""
    top = G.dense(300, seed=3, drop_edge=True)
    att = np.arange(300, dtype=np.int32)
    src, dst = _requests(att, n_src=300, n_dst=3)
    n_uniq = _n_uniq(src, dst)
    eng = E.Engine(top, att, force_mode=4)
    eng.set_paths_row_tier(True)
    ref = eng.get_paths(src, dst, hops=True)
    ref_info = eng.paths_info()
    eng.close()
    monkeypatch.setenv("SHDPE_DENSE_BATCH_GB", "0.0001")
    if paths_chunk:
        monkeypatch.setenv("SHDPE_PATHS_CHUNK", paths_chunk)
    eng = E.Engine(top, att, force_mode=4, debug_flags=E.DEBUG_ENV)
    eng.set_paths_row_tier(True)
    got = eng.get_paths(src, dst, hops=True)
    info = eng.paths_info()
    eng.close()
    _same_bytes(got, ref)
    assert ref_info["rows"] == n_uniq == 300
    if paths_chunk is None:
        assert info["rows"] == n_uniq
    assert info["emulated"] == info["handed_on"] == 0


# ---- 4. default and switches ----------------------------------------------------

@pytest.mark.parametrize("name", ["sparse_tiefree", "dense"])
def test_off_by_default_and_switches(E, name, monkeypatch):
    _, att, _, _, _ = _case(name)
    src, dst = _requests(att)
    n_uniq = _n_uniq(src, dst)
    eng = _engine(E, name, row_tier=False)                # never made the call: as before
    ref = eng.get_paths(src, dst, hops=True)
    info = eng.paths_info()
    assert info["rows"] == 0 and info["emulated"] == n_uniq and info["groups"] > 0
    for on in (True, False, True):                        # the counters follow the switch
        eng.set_paths_row_tier(on)
        _same_bytes(eng.get_paths(src, dst, hops=True), ref)
        info = eng.paths_info()
        assert (info["rows"], info["emulated"]) == ((n_uniq, 0) if on else (0, n_uniq)), on
    eng.close()
    monkeypatch.setenv("SHDPE_PATHS_FAST", "0")           # every fast tier off, this one too
    eng = _engine(E, name, debug_flags=E.DEBUG_ENV)
    _same_bytes(eng.get_paths(src, dst, hops=True), ref)
    info = eng.paths_info()
    eng.close()
    assert info["rows"] == 0 and info["emulated"] == n_uniq


def _inert_cases():
    batched = BASE_CASES["tiefree_batched"]
    latfold = BASE_CASES["latfold"]
    return {
        "batched": (batched[0], 5),
        "latfold": (latfold[0], latfold[2]),
        "force_mode_3": (lambda: G.random_sparse(800, 5, seed=34), 3),
        "complete": (lambda: Topology.load_npz(os.path.join(GOLDEN, "shipped_topology.npz"), name="shipped"), 0),
    }


@pytest.mark.parametrize("name", ["batched", "latfold", "force_mode_3", "complete"])
def test_inert_where_it_does_not_apply(E, name):
    """The call is accepted and changes nothing: same bytes, same counters, rows == 0."""
    make, force = _inert_cases()[name]
    top = make()
    att = np.arange(0, top.n, 3, dtype=np.int32)
    src, dst = _requests(att, n_src=30, n_dst=4)
    eng = E.Engine(top, att, force_mode=force)
    assert eng.is_complete == (name == "complete")
    ref = eng.get_paths(src, dst, hops=True)
    ref_info = eng.paths_info()
    eng.set_paths_row_tier(True)
    got = eng.get_paths(src, dst, hops=True)
    info = eng.paths_info()
    eng.close()
    _same_bytes(got, ref)
    assert info["rows"] == 0 and ref_info["rows"] == 0
    for key in ("batch", "tie", "emulated", "handed_on", "groups"):
        assert info[key] == ref_info[key], key


# ---- 5. no side effects ---------------------------------------------------------

@pytest.mark.parametrize("name", ["sparse_quantized", "dense_quantized"])
def test_no_side_effects(E, name):
    """Table bytes, ShdPeStats and the one-pair call's answers are what they
    were: the tier stores no row, and the slot-0 cache it overwrites is dropped."""
    _, att, _, _, _ = _case(name)
    eng = _engine(E, name)
    eng.compute_all()
    T = eng.T
    s, t, t2 = int(att[3]), int(att[50]), int(att[7])
    one = eng.get_path(s, t)
    before, ck = eng.stats(), eng.row_checksums(0, T)
    picks = [int(att[0]), s, int(att[-1])]
    rows = [eng.get_row(v) for v in picks]
    src, dst = _requests(att, n_src=att.shape[0], n_dst=3)
    eng.get_paths(src, dst, hops=True)
    info = eng.paths_info()
    assert info["rows"] > 0 and info["tie"] + info["emulated"] > 0      # every branch of the tier ran
    assert eng.stats() == before
    assert np.array_equal(eng.row_checksums(0, T), ck)
    for v, row in zip(picks, rows):
        after = eng.get_row(v)
        for key, val in row.items():
            assert val.tobytes() == after[key].tobytes(), (v, key)
    assert eng.get_path(s, t) == one
    eng.get_paths(src[:40], dst[:40])
    assert eng.get_path(s, t2) == eng.get_paths([s], [t2])[1].tolist()
    assert eng.stats() == before
    eng.close()


# ---- 6. two logical shards ------------------------------------------------------

def test_two_shards(E):
    name = "sparse_tiefree"
    _, att, _, _, _ = _case(name)
    src, dst = _requests(att, n_src=att.shape[0], n_dst=3)
    eng = _engine(E, name)
    ref = eng.get_paths(src, dst, hops=True)
    eng.close()
    eng = _engine(E, name, devices=[0, 0])
    got = eng.get_paths(src, dst, hops=True)
    info = eng.paths_info()
    bounds = eng.shard_bounds()
    eng.close()
    assert len(bounds) == 3 and 0 < bounds[1] < att.shape[0]
    _same_bytes(got, ref)
    assert info["rows"] == _n_uniq(src, dst) and info["emulated"] == 0
