"""CPU tests of the all-pairs load's parent tier at the C ABI
(shd_pe_table_load_set_parent_tier, shd_pe_table_load_info's entries 8 to 11):
declared in the header, exported by the library, bound by the ctypes table with
the header's types, refusing a NULL engine without touching a GPU, and its
kernel built for gfx950."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "shd_pathengine.h")
LIB = os.path.join(ROOT, "shadow-1_amd", "libshdpe.so")
SETTER = "shd_pe_table_load_set_parent_tier"
CTYPE = {"int32_t": C.c_int32, "int64_t": C.c_int64, "int": C.c_int}


@pytest.fixture(scope="module")
def E():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "shadow-1_amd")], check=True)
    from shdpe import engine
    engine.load_library()
    return engine


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_setter_declared_exported_and_bound(E):
    txt = _header()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (\w+)", out))
    lib = E.load_library()
    res, args = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)\s*;" % SETTER, txt).groups()
    assert re.fullmatch(r"\s*ShdPe\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*", args), args
    assert SETTER in exported
    assert SETTER in E.EXPORTS
    fn = getattr(lib, SETTER)
    assert fn.restype is CTYPE[res]
    assert list(fn.argtypes) == [C.c_void_p, C.c_int32]
    assert hasattr(E.Engine, "set_table_load_parent_tier")
    # the additions are listed under the version they were added at, which stays 16
    raw = open(HEADER).read()
    ver = re.search(r"#define\s+SHD_PE_ABI_VERSION\s+(\d+)\s*/\*(.*?)\*/", raw, flags=re.S)
    assert int(ver.group(1)) == 16
    assert SETTER in ver.group(2)


def test_null_engine_is_einval(E):
    lib = E.load_library()
    assert lib.shd_pe_table_load_set_parent_tier(None, 1) == E.EINVAL
    assert lib.shd_pe_table_load_set_parent_tier(None, 0) == E.EINVAL
    info = np.full(12, -7, np.int64)
    assert lib.shd_pe_table_load_info(None, info.ctypes.data_as(C.c_void_p), 12) == E.EINVAL
    assert np.all(info == -7)


def test_kernel_built_for_gfx950():
    data = open(LIB, "rb").read()
    assert b"gfx950" in data
    assert b"k_tree_load_parents" in data
