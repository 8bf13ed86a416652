"""CPU tests of the all-pairs load call's C ABI (shd_pe_table_load,
shd_pe_table_load_info): declared in the header at ABI 16, exported by the
library, bound by the ctypes table with the header's argument types, and
refusing NULL arguments without touching a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "shd_pathengine.h")
LIB = os.path.join(ROOT, "shadow-1_amd", "libshdpe.so")
NEW = ("shd_pe_table_load", "shd_pe_table_load_info")


@pytest.fixture(scope="module")
def E():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "shadow-1_amd")], check=True)
    from shdpe import engine
    engine.load_library()
    return engine


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_symbols_declared_exported_and_bound(E):
    txt = _header()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (\w+)", out))
    lib = E.load_library()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in exported, name
        assert name in E.EXPORTS, name
        assert getattr(lib, name).argtypes is not None, name


def test_abi_version_is_16():
    assert int(re.search(r"#define\s+SHD_PE_ABI_VERSION\s+(\d+)", _header()).group(1)) == 16


CTYPE = {"int32_t": C.c_int32, "int64_t": C.c_int64, "int": C.c_int}


def _ctype(decl):
    """The ctypes type of one C parameter or field declaration of the header."""
    decl = decl.strip()
    if "*" in decl:
        return C.c_void_p
    return CTYPE[decl.replace("const", "").split()[0]]


def test_binding_matches_header(E):
    """Argument and result types of both calls, and ShdPeTableLoadIn field by field."""
    txt = _header()
    lib = E.load_library()
    for name in NEW:
        res, args = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, txt).groups()
        fn = getattr(lib, name)
        assert fn.restype is CTYPE[res], name
        assert list(fn.argtypes) == [_ctype(a) for a in args.split(",")], name
    body = re.search(r"typedef struct ShdPeTableLoadIn\s*\{(.*?)\}\s*ShdPeTableLoadIn\s*;", txt, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        if "*" in decl:
            fields.append((decl.split("*")[-1].strip(), C.c_void_p))
            continue
        ty, names = decl.split(None, 1)
        fields += [(n.strip(), CTYPE[ty]) for n in names.split(",")]
    assert [(n, t) for n, t in E.TableLoadInC._fields_] == fields
    assert fields == [("start", C.c_int32), ("count", C.c_int32), ("weight", C.c_void_p), ("ld", C.c_int64)]
    assert C.sizeof(E.TableLoadInC) == 24


def test_kernels_built_for_gfx950():
    data = open(LIB, "rb").read()
    assert b"gfx950" in data
    assert b"k_tree_load" in data and b"k_table_direct" in data


def test_null_arguments_are_einval(E):
    """A NULL engine, `in` or `out` is refused before anything is written."""
    lib = E.load_library()
    arc, vert, totals = np.full(3, 7, np.uint64), np.full(3, 7, np.uint64), np.full(4, 7, np.uint64)
    info = np.full(8, 7, np.int64)
    o = E.LoadOutC(_vp(arc), _vp(vert), None, _vp(totals))
    i = E.TableLoadInC(0, 1, None, 0)
    assert lib.shd_pe_table_load(None, C.byref(i), C.byref(o)) == E.EINVAL
    assert lib.shd_pe_table_load_info(None, _vp(info), 8) == E.EINVAL
    # (a non-NULL handle is never dereferenced before `in` and `out` are looked at)
    buf = C.create_string_buffer(64)
    fake = C.c_void_p(C.addressof(buf))
    assert lib.shd_pe_table_load(fake, None, C.byref(o)) == E.EINVAL
    assert lib.shd_pe_table_load(fake, C.byref(i), None) == E.EINVAL
    assert lib.shd_pe_table_load_info(fake, None, 8) == E.EINVAL
    for a in (arc, vert, totals, info):
        assert np.all(a == 7)
