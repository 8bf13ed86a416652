"""CPU tests of the path extraction's row tier at the C ABI (ABI 13:
shd_pe_paths_set_row_tier, shd_pe_paths_info's seventh entry): declared in the
header, exported by the library, bound by the ctypes table, refusing a NULL
engine without touching a GPU, and its walk kernel built for gfx950."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "shd_pathengine.h")
SO = os.path.join(ROOT, "shadow-1_amd", "libshdpe.so")
NEW = ("shd_pe_paths_set_row_tier",)
NEW_KERNELS = (b"k_paths_walk_dense",)


@pytest.fixture(scope="module")
def E():
    if not os.path.exists(SO):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "shadow-1_amd")], check=True)
    from shdpe import engine
    engine.load_library()
    return engine


def test_symbol_declared_exported_and_bound(E):
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", SO], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (\w+)", out))
    lib = E.load_library()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(\s*ShdPe\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*\)" % name, txt), name
        assert name in exported, name
        assert name in E.EXPORTS, name
        assert getattr(lib, name).argtypes is not None, name
    assert int(re.search(r"#define\s+SHD_PE_ABI_VERSION\s+(\d+)", txt).group(1)) >= 13
    assert hasattr(E.Engine, "set_paths_row_tier")


def test_null_engine_is_einval(E):
    lib = E.load_library()
    assert lib.shd_pe_paths_set_row_tier(None, 1) == E.EINVAL
    assert lib.shd_pe_paths_set_row_tier(None, 0) == E.EINVAL
    info = np.full(7, -7, np.int64)
    assert lib.shd_pe_paths_info(None, info.ctypes.data_as(C.c_void_p), 7) == E.EINVAL
    assert np.all(info == -7)


def test_walk_kernel_built_for_gfx950(E):
    data = open(SO, "rb").read()
    assert b"gfx950" in data
    for k in NEW_KERNELS:
        assert k in data, k
        assert b"k_path_walk" not in k                    # (tests/test_paths_host.py forbids that substring)
    assert b"k_path_walk" not in data
