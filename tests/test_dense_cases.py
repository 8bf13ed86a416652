"""CPU test of the premises of the dense-path cases (dense_cases.py): every
graph has what its case in test_gpu_dense.py is there for, by the oracle
alone.  A later change to a generator must fail here rather than turn a GPU
test into one that passes without testing anything."""
import numpy as np
import pytest

import dense_cases as DC


@pytest.fixture(scope="module")
def cases(oracle_mod):
    out = {}
    for name in DC.ALL:
        top, att, force = DC.build(name)
        out[name] = (top, att, force, oracle_mod.OracleGraph(top))
    return out


@pytest.mark.parametrize("name", DC.ALL)
def test_not_complete_and_deterministic(cases, name):
    top, att, force, og = cases[name]
    assert not og.is_complete()            # Dijkstra rows, not direct ones
    again, att2, _ = DC.build(name)
    assert np.array_equal(att, att2)
    for k in ("src", "dst", "latency", "loss"):
        assert getattr(top, k).tobytes() == getattr(again, k).tobytes(), k
    # mode 3 by density (DENSE_MIN) or by forceMode 4; sparse ones must force it
    if name.startswith(("tiny", "sparse", "chain")):
        assert force == 4
    assert np.array_equal(np.unique(att), att) and att.min() >= 0 and att.max() < top.n


def test_sizes_sit_on_the_tile_edges():
    assert DC.TINY_N == (1, 2, 15, 16, 17)
    assert DC.EDGE_N == (127, 128, 129, 257)
    assert DC.ROWS_K == (31, 32, 33, 95, 96, 97)
    assert [n % 16 for n in DC.EDGE_N] == [15, 0, 1, 1]
    assert [n % 128 for n in DC.EDGE_N] == [127, 0, 1, 1]
    assert max(DC.ROWS_K) <= 129


@pytest.mark.parametrize("name", DC.TIE_UNDIRECTED + DC.TIE_DIRECTED)
def test_tie_cases_have_tie_rows(cases, name):
    top, att, _, og = cases[name]
    assert top.directed == (name in DC.TIE_DIRECTED)
    ties = DC.tie_rows(og, top, att)
    print(name, "tie rows", len(ties), "of", att.shape[0])
    assert len(ties) > 0


def test_dir129_is_tie_free(cases):
    top, att, _, og = cases["dir129"]
    assert top.directed and DC.tie_rows(og, top, att) == []


def test_directed_cases_are_asymmetric(cases):
    """A transposed W must change distances: the arc sets differ from their
    transposes and so do the oracle's rows."""
    for name in ("dir129", "dir129q", "dir257q_holes"):
        top, att, _, og = cases[name]
        W = DC.arc_matrix(top)
        assert np.isfinite(W).sum() > 0.5 * top.n * (top.n - 1)
        assert (np.isfinite(W) != np.isfinite(W.T)).any()
        d0 = DC.distances(og, 0)
        back = np.array([DC.distances(og, v)[0] for v in range(1, 6)])
        assert not np.array_equal(d0[1:6], back)


def test_holes_case(cases, oracle_mod):
    top, att, _, og = cases["dir257q_holes"]
    assert att.shape[0] < top.n                                # T < n
    assert np.diff(att).max() > 1                              # unattached vertices in between
    assert top.vloss is not None and np.any(top.vloss > 0)
    rows = og.rows(att, att, threads=4)
    fl = rows["flags"]
    assert np.any(fl & oracle_mod.F_UNREACHABLE) and np.any(fl & oracle_mod.F_NOEDGE)
    # the isolated vertices: unreachable from every other vertex, and attached
    iso = np.arange(top.n - 3, top.n)
    assert np.isin(iso, att).all() and np.isin(np.arange(5), att).all()
    pos = {int(v): k for k, v in enumerate(att)}
    assert fl[pos[3], pos[3]] & oracle_mod.F_NOEDGE
    assert fl[pos[0], pos[int(iso[0])]] & oracle_mod.F_UNREACHABLE
    assert not (fl[pos[int(iso[0])], pos[0]] & oracle_mod.F_UNREACHABLE)
    # the path test's requests hold reachable and unreachable pairs
    from test_gpu_paths import _requests
    src, dst = _requests(att)
    unreach = np.array([fl[pos[int(s)], pos[int(t)]] & oracle_mod.F_UNREACHABLE for s, t in zip(src, dst)])
    assert unreach.any() and not unreach.all()


def test_und97q_partial_attachment(cases):
    top, att, _, _ = cases["und97q"]
    assert not top.directed and top.n == 97 and att.shape[0] == 49


@pytest.mark.parametrize("name", ["sparse_q", "sparse_dir_q"])
def test_sparse_cases_have_low_degrees(cases, name):
    """Degrees below the 15 scan waves of k_exact_dense (empty segments) and
    below n - 1 (the tie export's binary-search branch)."""
    top, _, _, _ = cases[name]
    deg = np.bincount(top.src, minlength=top.n)
    if not top.directed:
        deg = deg + np.bincount(top.dst, minlength=top.n)
    assert deg.min() >= 1 and np.median(deg) < 15 and deg.max() < top.n - 1


def test_chain_is_deep(cases):
    top, att, _, og = cases["chain400"]
    row = og.row(0, att)
    assert row["hops"].max() == DC.CHAIN_N - 1
    assert top.vloss is not None
