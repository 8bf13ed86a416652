"""GPU tests of batched host attachment (k_attach, pe_attach.hip) against the
serial restatement of topology.c:2094-2369 (tests/attach_reference.py) and the
one-query host form."""
import os

import numpy as np
import pytest

import attach_reference as R
from conftest import GOLDEN
from shdpe import engine as E
from shdpe import generators as G

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257, 5000)        # one vertex, around one wave step, several steps
HOSTS = (1, 65, 1000)                     # one host, a partial last host group, many workgroups
FIELDS = R.FIELDS


def _as_rows(out, count):
    return [{k: out[k][i].item() for k in FIELDS} for i in range(count)]


@pytest.fixture(scope="module")
def grid():
    """Per (V, hosts): va, hints, the serial reference and the device result,
    each computed once."""
    cases = {}
    for vi, n in enumerate(SIZES):
        va = G.vertex_attrs(n, seed=500 + vi)
        lists = R.vertex_lists(va)
        at = E.Attacher(va)
        for hi, count in enumerate(HOSTS):
            h = G.attach_hints(va, count, seed=700 + 10 * vi + hi)
            want = [R.serial(va, h, i, lists) for i in range(count)]
            cases[(n, count)] = (va, h, want, at.attach(h))
        at.close()
    return cases


@pytest.mark.parametrize("count", HOSTS)
@pytest.mark.parametrize("n", SIZES)
def test_batched_matches_serial_restatement(grid, n, count):
    va, h, want, out = grid[(n, count)]
    got = _as_rows(out, count)
    bad = [i for i in range(count) if got[i] != want[i]]
    assert not bad, (n, count, bad[:5], got[bad[0]], want[bad[0]])


def test_grid_covers_every_set_and_mode(grid):
    seen = set()
    for va, h, want, out in grid.values():
        seen |= R.combos_of(out)
    assert sorted(seen) == list(range(R.N_COMBOS))


@pytest.mark.parametrize("n", SIZES)
def test_batched_matches_attach_host(grid, n):
    for count in HOSTS:
        va, h, _, out = grid[(n, count)]
        got = _as_rows(out, count)
        for i in range(count):
            assert got[i] == E.attach_host(va, h, i), (n, count, i)


def test_crafted_edge_cases_on_device():
    for name, va, h, vertex, cset, used in R.crafted_cases():
        want = R.serial(va, h, 0)
        assert (want["vertex"], want["candidate_set"], want["used_random"]) == (vertex, cset, used), name
        at = E.Attacher(va)
        # alone, and as every host of three groups (each wave slot sees it)
        assert _as_rows(at.attach(h), 1) == [want], name
        many = {k: np.repeat(np.asarray(v), 11) for k, v in h.items()}
        assert _as_rows(at.attach(many), 11) == [want] * 11, name
        at.close()


def test_hosts_without_hints_take_the_ordinal():
    """Every host of a wave in set 7 / random: the walks 2 and 3 are skipped."""
    va = G.vertex_attrs(1000, seed=11)
    count = 37
    rng = np.random.default_rng(12)
    none = np.full(count, -1, np.int32)
    h = dict(ip_given=np.zeros(count, np.uint8), ip=np.zeros(count, np.uint32), citycode=none,
             countrycode=none, geocode=none, type=none, random=rng.random(count))
    h["random"][:3] = (0.0, 1.0, 0.5)
    at = E.Attacher(va)
    out = at.attach(h)
    at.close()
    assert _as_rows(out, count) == [R.serial(va, h, i) for i in range(count)]
    assert out["vertex"][:3].tolist() == [0, 999, 500] and set(out["candidate_set"].tolist()) == {7}


def test_large_table_matches_order_free_form():
    n, count = 100_000, 512
    va = G.vertex_attrs(n, seed=21, n_city=40, n_country=12, n_geo=5, n_type=3)
    # vertex 99,999 alone carries 10.77.0.1; vertex 0 alone carries type 7
    va.ip[va.ip == G.ip_raw("10.77.0.1")] = R.NONE
    va.ip[n - 1] = G.ip_raw("10.77.0.1")
    va.type[0] = 7
    h = G.attach_hints(va, count, seed=22)
    h["ip_given"][0], h["ip"][0] = 1, G.ip_raw("10.77.0.1")
    for k in ("citycode", "countrycode", "geocode"):
        h[k][1] = -1
    h["type"][1], h["ip_given"][1] = 7, 0
    at = E.Attacher(va)
    out = at.attach(h)
    at.close()
    got = _as_rows(out, count)
    assert (got[0]["vertex"], got[0]["candidate_set"], got[0]["num_candidates"]) == (n - 1, 8, 1)
    assert (got[1]["vertex"], got[1]["candidate_set"], got[1]["num_candidates"]) == (0, 6, 1)
    for i in range(count):
        assert got[i] == R.order_free(va, h, i), i


def test_staging_chunks_give_identical_results():
    va = G.vertex_attrs(300, seed=31)
    h = G.attach_hints(va, 1000, seed=32)
    one = E.Attacher(va)
    ref = one.attach(h)
    one.close()
    for chunk in (1, 7, 256, 999):
        at = E.Attacher(va, chunk=chunk)
        out = at.attach(h)
        at.close()
        for k in FIELDS:
            assert np.array_equal(out[k], ref[k]), (chunk, k)


def test_bad_random_double_is_refused_before_any_work():
    va = G.vertex_attrs(10, seed=1)
    h = G.attach_hints(va, 4, seed=2)
    at = E.Attacher(va)
    for bad in (-0.5, 1.5, float("nan")):
        with pytest.raises(E.EngineError) as ei:
            at.attach(dict(h, random=np.array([0.5, 0.5, 0.5, bad])))
        assert ei.value.code == E.EINVAL
    assert at.attach(h)["vertex"].shape == (4,)
    at.close()


def test_shipped_graphml_attach_to_engine(oracle_mod):
    """parse -> vertex attrs -> attach -> Engine: hosts hinted by country code
    land on that country's single vertex, hosts hinted by address on the vertex
    that has it; the unique vertices feed the path engine."""
    path = os.path.join(GOLDEN, "topology.graphml.xml.xz")
    va = E.parse_graphml_vertex_attrs(path)
    top = E.parse_graphml(path)
    rng = np.random.default_rng(5)
    count = 64
    verts = rng.choice(va.n, count, replace=True)
    cc = np.array([va.attr_code(E.VATTR_COUNTRYCODE, va.attr_string(int(v), E.VATTR_COUNTRYCODE).lower())
                   for v in verts], np.int32)
    assert np.array_equal(cc, va.countrycode[verts])
    none = np.full(count, -1, np.int32)
    h = dict(ip_given=np.zeros(count, np.uint8), ip=np.zeros(count, np.uint32), citycode=none.copy(),
             countrycode=cc, geocode=none.copy(), type=none.copy(), random=rng.random(count))
    h["type"][::2] = va.attr_code(E.VATTR_TYPE, "cluster")
    # the last four by address instead: exact matches
    u, c = np.unique(va.ip, return_counts=True)
    with_ip = [v for v in np.flatnonzero((va.ip != 0) & (va.ip != R.NONE)) if va.ip[v] in u[c == 1]][:4]
    assert len(with_ip) == 4
    for j, v in enumerate(with_ip):
        i = count - 4 + j
        verts[i] = v
        h["countrycode"][i], h["ip_given"][i], h["ip"][i] = -1, 1, va.ip[v]
    at = E.Attacher(va)
    out = at.attach(h)
    at.close()
    assert np.array_equal(out["vertex"], verts)
    assert set(out["candidate_set"][:count - 4].tolist()) <= {2, 3}
    assert set(out["candidate_set"][count - 4:].tolist()) == {8}
    assert np.array_equal(out["bw_down"], va.bandwidth_down[verts].astype(np.uint64))
    assert np.array_equal(out["bw_up"], va.bandwidth_up[verts].astype(np.uint64))
    _, first = np.unique(out["vertex"], return_index=True)
    attached = out["vertex"][np.sort(first)]                     # first-occurrence order
    eng = E.Engine(top, attached)
    assert np.array_equal(eng.attached, attached)
    s = int(attached[3])
    eng.compute_rows([s])
    got = eng.get_row(s)
    og = oracle_mod.OracleGraph(top)
    assert eng.is_complete and np.all(got["flags"] == E.F_DIRECT)       # complete graph: the direct-edge row
    for j, t in enumerate(eng.attached):
        lat, rel = og.direct(s, int(t))
        assert got["lat"][j] == lat and got["rel"][j] == rel, (s, t)
    eng.close()
    va.close()
