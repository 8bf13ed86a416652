"""CPU tests of the link / vertex load calls' C ABI (shd_pe_path_load, the arc
list, shd_topology_link_load): declared in the header, exported by the library,
bound by the ctypes table, refusing NULL arguments without touching a GPU; and
the numpy helper that folds arc loads onto the topology's edges."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from shdpe.graph import Topology

HEADER = os.path.join(ROOT, "include", "shd_pathengine.h")
LIB = os.path.join(ROOT, "shadow-1_amd", "libshdpe.so")
NEW = ("shd_pe_num_arcs", "shd_pe_arc_list", "shd_pe_find_arc", "shd_pe_path_load",
       "shd_pe_path_load_info", "shd_topology_link_load")


@pytest.fixture(scope="module")
def E():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "shadow-1_amd")], check=True)
    from shdpe import engine
    engine.load_library()
    return engine


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def test_symbols_declared_exported_and_bound(E):
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (\w+)", out))
    lib = E.load_library()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in exported, name
        assert name in E.EXPORTS, name
        assert getattr(lib, name).argtypes is not None, name
    assert "typedef struct ShdPeLoadOut" in txt
    assert int(re.search(r"#define\s+SHD_PE_ABI_VERSION\s+(\d+)", txt).group(1)) >= 14


def test_load_out_struct_layout(E):
    """ShdPeLoadOut: four pointers, in the header's order."""
    assert [f for f, _ in E.LoadOutC._fields_] == ["arcLoad", "vertexLoad", "status", "totals"]
    assert C.sizeof(E.LoadOutC) == 4 * 8


def test_kernel_built_for_gfx950(E):
    data = open(LIB, "rb").read()
    assert b"gfx950" in data
    assert b"k_paths_load" in data
    assert b"k_path_walk" not in data


def test_null_arguments_are_einval(E):
    """A NULL engine or a NULL `out` is refused before anything is written."""
    lib = E.load_library()
    src = np.zeros(2, np.int32)
    w = np.ones(2, np.uint64)
    arc, vert = np.full(3, 7, np.uint64), np.full(3, 7, np.uint64)
    status, totals = np.full(2, 7, np.int32), np.full(4, 7, np.uint64)
    o = E.LoadOutC(_vp(arc), _vp(vert), _vp(status), _vp(totals))
    assert lib.shd_pe_path_load(None, _vp(src), _vp(src), _vp(w), 2, C.byref(o)) == E.EINVAL
    assert lib.shd_topology_link_load(None, C.byref(o)) == E.EINVAL
    for a in (arc, vert, status, totals):
        assert np.all(a == 7)
    # (a non-NULL handle is never dereferenced before `out` is looked at)
    buf = C.create_string_buffer(64)
    fake = C.c_void_p(C.addressof(buf))
    assert lib.shd_pe_path_load(fake, _vp(src), _vp(src), None, 2, None) == E.EINVAL
    assert lib.shd_topology_link_load(fake, None) == E.EINVAL
    assert lib.shd_pe_num_arcs(None) == 0
    assert lib.shd_pe_arc_list(None, _vp(src), _vp(src)) == E.EINVAL
    assert lib.shd_pe_find_arc(None, 0, 1) == -1


def _multigraph(directed):
    # edge:        0       1       2       3       4       5
    #              0-1     1-0     2-2     1-2     2-3     1-2 (newest of 1-2)
    src = np.array([0, 1, 2, 1, 2, 1], np.int32)
    dst = np.array([1, 0, 2, 2, 3, 2], np.int32)
    return Topology(n=4, directed=directed, src=src, dst=dst, latency=np.ones(6), loss=np.zeros(6))


def _arcs(top):
    """The merged non-loop OUT arcs, sorted by (from, to), as the engine lists them."""
    pairs = set()
    for a, b in zip(top.src.tolist(), top.dst.tolist()):
        if a == b:
            continue
        pairs.add((a, b))
        if not top.directed:
            pairs.add((b, a))
    pairs = sorted(pairs)
    return np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32)


def test_edge_load_directed(E):
    """Directed: 0->1 and 1->0 are two groups; the two 1->2 edges are one, the
    newest (5) takes it; the self-loop and the older parallel edge get 0; 2->3
    carries no load."""
    top = _multigraph(True)
    af, at = _arcs(top)
    assert list(zip(af.tolist(), at.tolist())) == [(0, 1), (1, 0), (1, 2), (2, 3)]
    load = np.array([5, 7, 2 ** 40 + 1, 0], np.uint64)
    got = E.edge_load(top, af, at, load)
    assert got.dtype == np.uint64
    assert got.tolist() == [5, 7, 0, 0, 0, 2 ** 40 + 1]


def test_edge_load_undirected(E):
    """Undirected: 0-1 and 1-0 are one group whatever their orientation, the
    newest (edge 1) takes the sum of both arcs; likewise edge 5 for 1-2."""
    top = _multigraph(False)
    af, at = _arcs(top)
    assert list(zip(af.tolist(), at.tolist())) == [(0, 1), (1, 0), (1, 2), (2, 1), (2, 3), (3, 2)]
    load = np.array([5, 7, 11, 2 ** 63, 0, 0], np.uint64)
    got = E.edge_load(top, af, at, load)
    assert got.tolist() == [0, 12, 0, 0, 0, 2 ** 63 + 11]
    # sums stay modulo 2**64
    load[2] = 2 ** 63
    assert E.edge_load(top, af, at, load)[5] == 0
