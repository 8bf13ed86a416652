"""CPU tests of host attachment (topology_attach, topology.c:2094-2430): the
vertex attributes the GraphML reader keeps, and shd_pe_attach_host against the
serial restatement of the reference rule (tests/attach_reference.py)."""
import os

import numpy as np
import pytest

import attach_reference as R
from conftest import GOLDEN
from shdpe import engine as E
from shdpe import generators as G

SHIPPED = os.path.join(GOLDEN, "topology.graphml.xml.xz")
SIZES = (1, 2, 63, 64, 65, 130, 257)
VAS_PER_SIZE, HOSTS_PER_VA = 10, 43          # 7 * 10 * 43 = 3,010 cases


def _usable(ip):
    return (ip != R.NONE) & (ip != R.ANY) & (ip != R.LOOPBACK)


def test_shipped_topology_vertex_attrs():
    va = E.parse_graphml_vertex_attrs(SHIPPED)
    assert va.n == 183
    assert va.citycode is None and va.geocode is None
    assert len(set(va.countrycode.tolist())) == 183 and va.countrycode.min() == 0
    assert set(va.type.tolist()) == {0} and va.attr_code(E.VATTR_TYPE, "cluster") == 0
    assert va.attr_code(E.VATTR_TYPE, "CLUSTER") == 0
    us = _usable(va.ip)
    assert int(us.sum()) == 18
    assert set(va.ip[~us].tolist()) == {0}                        # the rest is 0.0.0.0
    assert va.ip[1] == G.ip_raw("190.181.151.39") and va.attr_string(1, E.VATTR_IP) == b"190.181.151.39"
    assert va.bandwidth_down[0] == 1711.0 and va.bandwidth_up[0] == 886.0
    assert va.bandwidth_down[1] == 2830.0 and va.bandwidth_up[1] == 1814.0
    assert np.all(va.bandwidth_down == np.floor(va.bandwidth_down)) and not np.isnan(va.bandwidth_up).any()
    assert va.attr_string(0, E.VATTR_COUNTRYCODE) == b"SD"
    assert va.attr_code(E.VATTR_COUNTRYCODE, "sd") == va.countrycode[0]
    assert va.attr_string(0, E.VATTR_CITYCODE) is None
    va.close()


CRAFTED = """<?xml version="1.0"?>
<graphml>
  <key attr.name="countrycode" attr.type="string" for="node" id="c"/>
  <key attr.name="citycode" attr.type="string" for="node" id="y"/>
  <key attr.name="type" attr.type="string" for="node" id="t"><default>relay</default></key>
  <key attr.name="ip" attr.type="string" for="node" id="i"/>
  <key attr.name="bandwidthup" attr.type="double" for="node" id="u"><default>77</default></key>
  <key attr.name="bandwidthdown" attr.type="double" for="node" id="d"/>
  <key attr.name="geocode" attr.type="string" for="edge" id="g"/>
  <key attr.name="latency" attr.type="double" for="edge" id="l"/>
  <graph edgedefault="undirected">
    <node id="a"><data key="c">US</data><data key="y">N&amp;Y</data><data key="i">1.2.3.4</data><data key="d">5.5</data></node>
    <node id="b"><data key="c">us</data><data key="y">n&#38;y</data><data key="i">1.2.3.999</data><data key="u">12</data></node>
    <node id="c"><data key="c">Us</data><data key="y"></data><data key="t">Server</data><data key="i">127.0.0.1</data></node>
    <node id="d"><data key="c">\xc3\x9cs</data><data key="t"/><data key="i">1.0.0.127</data></node>
    <node id="e"><data key="c">\xc3\xbcs</data><data key="y">&lt;x&gt;</data></node>
    <edge source="a" target="b"><data key="l">1.0</data></edge>
  </graph>
</graphml>
""".encode("latin-1")


def test_crafted_graphml_vertex_attrs():
    va = E.parse_graphml_vertex_attrs(CRAFTED)
    assert va.n == 5
    cc = va.countrycode.tolist()
    assert cc[0] == cc[1] == cc[2] >= 0                          # US / us / Us: one code
    assert cc[3] >= 0 and cc[4] >= 0 and len({cc[0], cc[3], cc[4]}) == 3   # non-ASCII bytes are not folded
    assert va.attr_string(2, E.VATTR_COUNTRYCODE) == b"Us"
    city = va.citycode.tolist()
    assert city[0] == city[1] >= 0 and city[2] == -1 and city[3] == -1     # entities decoded; empty = absent
    assert va.attr_string(0, E.VATTR_CITYCODE) == b"N&Y" and va.attr_string(2, E.VATTR_CITYCODE) is None
    assert va.attr_string(4, E.VATTR_CITYCODE) == b"<x>" and city[4] not in (-1, city[0])
    assert va.attr_code(E.VATTR_CITYCODE, "n&y") == city[0]
    ty = va.type.tolist()                                          # <default>relay</default>
    assert ty[0] == ty[1] == ty[4] == va.attr_code(E.VATTR_TYPE, "RELAY") >= 0
    assert ty[2] == va.attr_code(E.VATTR_TYPE, "server") >= 0 and ty[2] != ty[0]
    assert va.attr_string(0, E.VATTR_TYPE) == b"relay"
    assert va.geocode is None                                      # the geocode key is an edge key
    assert va.ip.tolist() == [G.ip_raw("1.2.3.4"), R.NONE, 0x0100007F, 0x7F000001, R.NONE]
    assert _usable(va.ip).tolist() == [True, False, True, False, False]
    assert va.bandwidth_up.tolist() == [77.0, 12.0, 77.0, 77.0, 77.0]
    assert va.bandwidth_down[0] == 5.5 and np.isnan(va.bandwidth_down[1:]).all()
    # hints into the code space: NULL -> -1, empty / unknown -> -2, else the code
    assert va.attr_code(E.VATTR_COUNTRYCODE, None) == -1
    assert va.attr_code(E.VATTR_COUNTRYCODE, "") == -2
    assert va.attr_code(E.VATTR_COUNTRYCODE, "DE") == -2
    assert va.attr_code(E.VATTR_COUNTRYCODE, "uS") == cc[0]
    assert va.attr_code(E.VATTR_GEOCODE, "x") == -2
    # the existing results are unchanged
    top = E.parse_graphml(CRAFTED)
    assert top.n == 5 and top.m == 1 and top.latency.tolist() == [1.0]
    va.close()


@pytest.fixture(scope="module")
def random_cases():
    """(va, hints, lists) per generated vertex table; 3,010 hosts in all."""
    out = []
    for si, n in enumerate(SIZES):
        for k in range(VAS_PER_SIZE):
            va = G.vertex_attrs(n, seed=1000 + 37 * si + k)
            out.append((va, G.attach_hints(va, HOSTS_PER_VA, seed=9000 + 37 * si + k), R.vertex_lists(va)))
    return out


@pytest.fixture(scope="module")
def serial_results(random_cases):
    return [[R.serial(va, h, i, lists) for i in range(HOSTS_PER_VA)] for va, h, lists in random_cases]


def test_attach_host_matches_serial_restatement(random_cases, serial_results):
    total = 0
    for (va, h, _), want in zip(random_cases, serial_results):
        for i in range(HOSTS_PER_VA):
            got = E.attach_host(va, h, i)
            assert got == want[i], (va.n, i, got, want[i])
            total += 1
    assert total >= 3000


def test_random_cases_cover_every_set_and_mode(serial_results):
    seen = {}
    for want in serial_results:
        for res in want:
            seen[R.combo(res)] = seen.get(R.combo(res), 0) + 1
    assert sorted(seen) == list(range(R.N_COMBOS)), seen


def test_order_free_form_matches_serial(random_cases, serial_results):
    for (va, h, _), want in zip(random_cases, serial_results):
        for i in range(HOSTS_PER_VA):
            assert R.order_free(va, h, i) == want[i], (va.n, i)


@pytest.mark.parametrize("case", R.crafted_cases(), ids=lambda c: c[0])
def test_crafted_edge_cases(case):
    _, va, h, vertex, cset, used = case
    want = R.serial(va, h, 0)
    assert (want["vertex"], want["candidate_set"], want["used_random"]) == (vertex, cset, used)
    assert E.attach_host(va, h, 0) == want
    assert R.order_free(va, h, 0) == want


def test_generator_pools_hold_the_special_values():
    va = G.vertex_attrs(5000, seed=3)
    for s in ("0.0.0.0", "127.0.0.1", "1.0.0.127", "254.253.252.251"):
        assert (va.ip == G.ip_raw(s)).any(), s
    assert G.ip_raw("127.0.0.1") == 0x0100007F and G.ip_raw("1.0.0.127") == 0x7F000001
    assert G.ip_raw("not-an-address") == R.NONE and (va.ip == R.NONE).any()
    h = G.attach_hints(va, 2000, seed=4)
    assert (h["ip"][h["ip_given"] != 0] == G.ip_raw("1.2.3.4")).any()
    for r in (0.0, 0.5, 1.0):
        assert (h["random"] == r).any()
    for k in ("citycode", "countrycode", "geocode", "type"):
        assert {-1, -2, 0} <= set(h[k].tolist())


def test_attach_errors():
    va = G.vertex_attrs(10, seed=1)
    h = G.attach_hints(va, 4, seed=2)
    empty = E.VertexAttrs(0)
    with pytest.raises(E.EngineError) as ei:
        E.attach_host(empty, h, 0)
    assert ei.value.code == E.EINVAL
    with pytest.raises(E.EngineError) as ei:
        E.Attacher(empty)
    assert ei.value.code == E.EINVAL
    for bad in (-0.001, 1.0000001, float("nan"), float("inf")):
        hb = dict(h, random=np.array([0.5, bad, 0.5, 0.5]))
        with pytest.raises(E.EngineError) as ei:
            E.attach_host(va, hb, 1)
        assert ei.value.code == E.EINVAL
    for i in (-1, 4):
        with pytest.raises(E.EngineError) as ei:
            E.attach_host(va, h, i)
        assert ei.value.code == E.EINVAL


def test_attacher_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(E.EngineError) as ei:
        E.Attacher(G.vertex_attrs(10, seed=1))
    assert ei.value.code == E.ENODEV
