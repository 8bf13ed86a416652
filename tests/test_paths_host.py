"""CPU tests of the batched path extraction's C ABI (shd_pe_get_paths,
shd_pe_paths_info): declared in the header, exported by the library, bound by
the ctypes table, and refusing a NULL engine without touching a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "shd_pathengine.h")
NEW = ("shd_pe_get_paths", "shd_pe_paths_info")


@pytest.fixture(scope="module")
def E():
    so = os.path.join(ROOT, "shadow-1_amd", "libshdpe.so")
    if not os.path.exists(so):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "shadow-1_amd")], check=True)
    from shdpe import engine
    engine.load_library()
    return engine


def test_symbols_declared_exported_and_bound(E):
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "shadow-1_amd", "libshdpe.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (\w+)", out))
    lib = E.load_library()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in exported, name
        assert name in E.EXPORTS, name
        assert getattr(lib, name).argtypes is not None, name
    assert "typedef struct ShdPePathsOut" in txt
    assert int(re.search(r"#define\s+SHD_PE_ABI_VERSION\s+(\d+)", txt).group(1)) >= 6


def test_kernels_built_for_gfx950(E):
    """hipcc --offload-arch=gfx950 builds the library clean (an up-to-date make
    is a no-op) and its code object carries the extraction's kernels."""
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "shadow-1_amd")], check=True)
    data = open(os.path.join(ROOT, "shadow-1_amd", "libshdpe.so"), "rb").read()
    assert b"gfx950" in data
    for k in (b"k_paths_size", b"k_paths_scan", b"k_paths_hops", b"k_paths_flags", b"k_paths_walk_dist"):
        assert k in data, k
    assert re.search(rb"k_paths_walk(?!_dist)", data)     # (not only as the prefix of k_paths_walk_dist)
    assert b"k_path_walk" not in data                     # the one-pair call's own walk kernel is gone


def test_paths_out_struct_layout(E):
    """ShdPePathsOut: five pointers and the capacity, in the header's order."""
    names = [f for f, _ in E.PathsOutC._fields_]
    assert names == ["offsets", "verts", "hopLat", "hopRel", "status", "cap"]
    assert C.sizeof(E.PathsOutC) == 6 * 8


def test_null_engine_is_einval(E):
    lib = E.load_library()
    src = np.zeros(2, np.int32)
    offsets = np.full(3, -7, np.int64)
    o = E.PathsOutC(offsets.ctypes.data_as(C.c_void_p), None, None, None, None, 0)
    assert lib.shd_pe_get_paths(None, src.ctypes.data_as(C.c_void_p), src.ctypes.data_as(C.c_void_p),
                                2, C.byref(o)) == E.EINVAL
    assert np.all(offsets == -7)
    info = np.zeros(6, np.int64)
    assert lib.shd_pe_paths_info(None, info.ctypes.data_as(C.c_void_p), 6) == E.EINVAL
